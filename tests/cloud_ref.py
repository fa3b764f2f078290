"""numpy restatement of the point-cloud neighbour statistics (include/sfmx_cloud.h), shared by the cloud tests.

The distance of a point is FLANN's L2_Simple<float> restated operation by operation in np.float32
(dx = xi - xj; d = (dx*dx + dy*dy) + dz*dz, no FMA), reduced to z = #{d == 0} and m = min{d > 0};
statistics are MathUtils::calculateStatistics with sequential double sums; the three writers return
the files' bytes.  Nothing here calls the library.
"""
import math
import struct

import numpy as np


def _d_rows(x, i0, i1):
    """float32 d of points i0..i1 against all points: (i1 - i0) x n."""
    a = x[i0:i1, None, :]
    b = x[None, :, :]
    with np.errstate(over="ignore", invalid="ignore"):
        dx = a[..., 0] - b[..., 0]
        dy = a[..., 1] - b[..., 1]
        dz = a[..., 2] - b[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def neighbor_distances(xyz, max_equal=0):
    """-> (distance float64 (n), neighbor int64 (n)).  Non-finite points are never candidates; their own
    distance is 0 and their neighbour -1.  n <= 1 gives 0 / -1."""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(x)
    dist = np.zeros(n, np.float64)
    nb = np.full(n, -1, np.int64)
    if n <= 1:
        return dist, nb
    ke = min(2 + max(0, int(max_equal)), n)
    finite = np.isfinite(x).all(axis=1)
    step = max(1, (1 << 22) // n)
    for i0 in range(0, n, step):
        i1 = min(n, i0 + step)
        d = _d_rows(x, i0, i1)
        d[:, ~finite] = np.nan                       # never candidates
        z = (d == 0).sum(axis=1)
        pos = np.where(d > 0, d, np.float32(np.inf))
        m = pos.min(axis=1)
        has = (d > 0).any(axis=1)
        first = np.argmax((d > 0) & (pos == m[:, None]), axis=1)   # the smallest index attaining m
        ok = finite[i0:i1] & has & (z < ke)
        dist[i0:i1] = np.where(ok, np.sqrt(m.astype(np.float64)), 0.0)
        nb[i0:i1] = np.where(ok, first, -1)
    return dist, nb


def neighbor_distances_literal(xyz, max_equal=0):
    """The reference's literal form: the K = 2 + maxEqual smallest d (a stable sort), the first whose
    sqrt((double)d) is > 0, else 0.  Finite points only."""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(x)
    out = np.zeros(n, np.float64)
    if n <= 1:
        return out
    k = min(2 + max(0, int(max_equal)), n)
    for i in range(n):
        d = np.sort(_d_rows(x, i, i + 1)[0], kind="stable")[:k]
        for v in d:
            s = math.sqrt(float(v))
            if s > 0:
                out[i] = s
                break
    return out


def statistics(distances, n_points=None):
    d = np.sort(np.asarray(distances, np.float64).reshape(-1))
    n = len(d)
    s = dict(n_points=int(n if n_points is None else n_points), max=0.0, min=0.0, mean=0.0, median=0.0, variance=0.0,
             deviation=0.0)
    if n == 0:
        return s
    s["min"] = float(min(0.0, d.min()))
    s["max"] = float(max(0.0, d.max()))
    mean = float(np.add.accumulate(d)[-1]) / float(n)          # sequential, in sorted order
    with np.errstate(divide="ignore", invalid="ignore"):
        e = d - mean
        var = np.float64(np.add.accumulate(e * e)[-1]) / np.float64(float(n) - 1.0)
    s["mean"] = mean
    s["variance"] = float(var)
    s["deviation"] = float(np.sqrt(var))
    s["median"] = float((d[n // 2] + d[n // 2 - 1]) / 2.0) if n % 2 == 0 else float(d[n // 2])
    return s


def histogram(distances, resolution=-1.0):
    d = np.asarray(distances, np.float64).reshape(-1)
    if resolution < 0:
        resolution = statistics(d)["variance"]
    with np.errstate(divide="ignore", invalid="ignore"):
        key = d.copy() if resolution <= 0 else np.ceil(d / resolution) * resolution
    nan = int(np.isnan(key).sum())
    k, c = np.unique(key[~np.isnan(key)], return_counts=True)
    if nan:
        k, c = np.append(k, np.nan), np.append(c, nan)
    return k.astype(np.float64), c.astype(np.uint64)


def fmt6(v):
    """ostream << fixed / printf("%.6f") as glibc prints it: a NaN keeps its sign ("-nan" for the x86 default NaN)."""
    v = float(v)
    if math.isnan(v):
        return "-nan" if np.signbit(v) else "nan"
    return "%.6f" % v


def stats_csv(s):
    head = "N_Points,Max_Distance,Min_Distance,Avg_Distance,Median_Distance,Variance_Distance,Deviation_Distance\n"
    vals = ",".join(fmt6(s[k]) for k in ("max", "min", "mean", "median", "variance", "deviation"))
    return (head + "%d,%s\n" % (s["n_points"], vals)).encode()


def neighbors_csv(keys, counts):
    return ("Distance,Count\n" + "".join("%s,%d\n" % (fmt6(k), int(c)) for k, c in zip(keys, counts))).encode()


def to_u8(v):
    """double -> u_char as an x86-64 build converts it: truncation to int32 (0x80000000 for NaN or out of
    range), low 8 bits."""
    v = float(v)
    if not (-2147483649.0 < v < 2147483648.0):
        return 0
    return int(v) & 0xFF


QUALITY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                  "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                  "property float quality\nelement face %d\nproperty list uchar int vertex_indices\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty float quality\nend_header\n")


def quality_ply(xyz, distances, face_sizes=(), face_indices=(), cutoff=-1.0):
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    d = np.array(distances, np.float64).reshape(-1)
    if cutoff > 0:
        d = np.where(d > cutoff, cutoff, d)
    maxd = 0.0
    for v in d:
        if v > maxd:
            maxd = float(v)
    flat = not maxd > 0
    out = bytearray((QUALITY_HEADER % (len(d), len(face_sizes))).encode())

    def ratio(v):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float64(v) / np.float64(maxd))

    for i, v in enumerate(d):
        r = ratio(v)
        b8 = 0 if flat else to_u8(255 * r)
        r8 = 0 if flat else to_u8(255 * (1.0 - r))
        out += struct.pack("<fffBBB", *x[i].tolist(), r8, 0, b8) + np.float32(v).tobytes()
    at = 0
    fi = np.asarray(face_indices, np.int64).reshape(-1)
    for cnt in np.asarray(face_sizes, np.int64).reshape(-1):
        idx = fi[at:at + cnt]
        at += cnt
        if cnt > 255 or cnt <= 0 or (idx < 0).any() or (idx >= len(d)).any():
            continue
        q = np.float32(0)
        r8 = b8 = 0
        for j in idx:
            q = np.float32(np.float64(q) + d[j])
            r = ratio(d[j])
            b8 = 0 if flat else to_u8(float(b8) + 255 * r)
            r8 = 0 if flat else to_u8(float(r8) + 255 * (1.0 - r))
        q = np.float32(q / np.float32(cnt))
        out += struct.pack("<B", cnt) + idx.astype("<i4").tobytes() + struct.pack("<BBB", r8 // int(cnt), 0, b8 // int(cnt))
        out += q.tobytes()
    return bytes(out)


# ---- inputs ------------------------------------------------------------------------------------------

PLY_TYPES = {"char": "b", "uchar": "B", "short": "h", "ushort": "H", "int": "i", "uint": "I", "float": "f", "double": "d"}


def write_ply(path, xyz, face_sizes=(), face_indices=(), binary=True, vertex_extra=(), face_extra=(), extra_element=None,
              list_name="vertex_indices", index_type="int", xyz_first=True, comments=True):
    """A minimal PLY writer for test inputs.  vertex_extra / face_extra: [(type, name, value)] scalar properties
    written after (xyz_first) or before x, y, z / after the list; extra_element: (name, count, [(type, name,
    value)]) written between the vertex and the face element."""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    fs = [int(v) for v in face_sizes]
    fi = [int(v) for v in face_indices]
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii")]
    if comments:
        head += ["comment written by tests/cloud_ref.py", "obj_info none"]
    vprops = [("float", "x"), ("float", "y"), ("float", "z")]
    extra = [(t, nm) for t, nm, _ in vertex_extra]
    head.append("element vertex %d" % len(x))
    head += ["property %s %s" % p for p in (vprops + extra if xyz_first else extra + vprops)]
    if extra_element:
        head.append("element %s %d" % extra_element[:2])
        head += ["property %s %s" % (t, nm) for t, nm, _ in extra_element[2]]
    if fs or face_extra:
        head.append("element face %d" % len(fs))
        head.append("property list uchar %s %s" % (index_type, list_name))
        head += ["property %s %s" % (t, nm) for t, nm, _ in face_extra]
    head.append("end_header")
    body = bytearray()

    def scalars(props):
        if binary:
            return b"".join(struct.pack("<" + PLY_TYPES[t], v) for t, _, v in props)
        return " ".join(repr(v) for _, _, v in props)

    for p in x:
        if binary:
            own = struct.pack("<fff", *p.tolist())
            body += own + scalars(vertex_extra) if xyz_first else scalars(vertex_extra) + own
        else:
            own = " ".join("%.9g" % v for v in p.tolist())
            ex = scalars(vertex_extra)
            body += ((own + " " + ex if xyz_first else ex + " " + own).strip() + "\n").encode()
    if extra_element:
        for _ in range(extra_element[1]):
            body += scalars(extra_element[2]) if binary else (scalars(extra_element[2]) + "\n").encode()
    at = 0
    for cnt in fs:
        idx = fi[at:at + cnt]
        at += cnt
        if binary:
            body += struct.pack("<B", cnt) + struct.pack("<%d%s" % (cnt, "i" if index_type == "int" else "I"), *idx)
            body += scalars(face_extra)
        else:
            body += (" ".join(str(v) for v in [cnt] + idx) + " " + scalars(face_extra)).strip().encode() + b"\n"
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode() + bytes(body))


def lattice_case(g=16, spacing=1.0, origin=(0.0, 0.0, 0.0), seed=None):
    """A g x g x g lattice (x fastest) whose answers are known analytically when spacing and origin are
    exactly representable: every distance is `spacing`, and the neighbour of point i is the smallest index
    among its up to six lattice neighbours.  seed: a permutation of the points (neighbours follow it).
    -> (xyz float32, distance float64, neighbor int64)."""
    k, j, i = np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij")
    ijk = np.stack([i.ravel(), j.ravel(), k.ravel()], 1)
    n = len(ijk)
    perm = np.arange(n) if seed is None else np.random.default_rng(seed).permutation(n)
    pos = np.empty(n, np.int64)          # pos[lattice id] = index in the permuted cloud
    pos[perm] = np.arange(n)
    xyz = (np.asarray(origin, np.float64) + ijk[perm] * float(spacing)).astype(np.float32)
    lid = lambda a: (a[:, 2] * g + a[:, 1]) * g + a[:, 0]
    best = np.full(n, n, np.int64)
    for ax in range(3):
        for s in (-1, 1):
            nbr = ijk.copy()
            nbr[:, ax] += s
            ok = (nbr[:, ax] >= 0) & (nbr[:, ax] < g)
            cand = np.where(ok, pos[lid(np.clip(nbr, 0, g - 1))], n)
            best = np.minimum(best, cand)
    nb = np.empty(n, np.int64)
    nb[pos] = best                        # best is indexed by lattice id
    return xyz, np.full(n, float(np.float32(spacing)), np.float64), nb
