"""Input files of the cloud host tests (tests/test_cloud_host.py, tests/test_cloud_host_san.py): PLY files the
reader of csrc/cloud_host.hpp takes, written by tests/cloud_ref.write_ply, and malformed ones it must refuse."""
import os
import struct

import numpy as np

import cloud_ref


def small_mesh(seed=4, n=37, faces=11):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, 3)).astype(np.float32)
    x[3] = (1e-30, -0.0, 3.5e20)
    fs = [int(v) for v in rng.integers(0, 6, size=faces)]      # sizes 0 .. 5
    fi = [int(v) for v in rng.integers(0, n, size=sum(fs))]
    return x, fs, fi


def good_files(d):
    """-> [(name, path, xyz, face_sizes, face_indices)]: ascii and binary, with and without faces, with extra
    vertex and face properties of several types, an extra scalar element, both list names and index types."""
    x, fs, fi = small_mesh()
    extra = dict(vertex_extra=[("uchar", "red", 200), ("double", "confidence", 0.25), ("short", "label", -3)],
                 face_extra=[("float", "quality", 1.5), ("uchar", "flags", 1)],
                 extra_element=("camera", 3, [("float", "focal", 2.5), ("int", "id", 7)]))
    out = []
    for binary in (True, False):
        tag = "bin" if binary else "ascii"
        for name, kw, faces in (("plain", {}, True), ("cloud", {}, False), ("extra", dict(extra, xyz_first=False), True),
                                ("extra_after", extra, True), ("uint", dict(list_name="vertex_index", index_type="uint"), True),
                                ("bare", dict(comments=False), True)):
            p = os.path.join(d, f"good_{tag}_{name}.ply")
            cloud_ref.write_ply(p, x, fs if faces else (), fi if faces else (), binary=binary, **kw)
            out.append((f"{tag}_{name}", p, x, fs if faces else [], fi if faces else []))
    p = os.path.join(d, "good_empty.ply")
    cloud_ref.write_ply(p, np.zeros((0, 3), np.float32))
    out.append(("empty", p, np.zeros((0, 3), np.float32), [], []))
    return out


def bad_files(d):
    """-> [(name, path)]: every one must give SFMX_EINVAL."""
    x, fs, fi = small_mesh()
    good_bin, good_ascii = os.path.join(d, "_src_bin.ply"), os.path.join(d, "_src_ascii.ply")
    cloud_ref.write_ply(good_bin, x, fs, fi, binary=True)
    cloud_ref.write_ply(good_ascii, x, fs, fi, binary=False)
    b, a = open(good_bin, "rb").read(), open(good_ascii, "rb").read()
    hb = b.index(b"end_header\n") + len(b"end_header\n")
    vertex_only = (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\n"
                   b"property float z\n")
    two = struct.pack("<6f", 0, 0, 0, 1, 1, 1)
    face_head = b"element face 1\nproperty list uchar int vertex_indices\n"
    cases = {
        "big_endian": b.replace(b"binary_little_endian", b"binary_big_endian"),
        "x_double": b.replace(b"property float x", b"property double x"),
        "no_z": b.replace(b"property float z", b"property float w"),
        "second_list": vertex_only + face_head + b"property list uchar int texcoord\nend_header\n" + two + b"\x00\x00",
        "list_in_vertex": vertex_only + b"property list uchar int tags\nend_header\n" + two,
        "list_in_other": vertex_only + b"element edge 1\nproperty list uchar int ends\nend_header\n" + two + b"\x00",
        "count_type_int": vertex_only + b"element face 1\nproperty list int int vertex_indices\nend_header\n" + two
                          + struct.pack("<i", 0),
        "index_type_short": vertex_only + b"element face 1\nproperty list uchar short vertex_indices\nend_header\n" + two + b"\x00",
        "truncated_vertices": b[:hb + 12 * len(x) - 5],
        "truncated_faces": b[:-3],
        "vertex_count_overruns": b.replace(b"element vertex %d" % len(x), b"element vertex 99999999999"),
        "face_count_overruns": b.replace(b"element face %d" % len(fs), b"element face 4000000000"),
        "face_list_overruns": vertex_only + face_head + b"end_header\n" + two + b"\xc8" + struct.pack("<3i", 0, 1, 0),
        "ascii_truncated": a[:len(a) - 20],
        "ascii_negative_count": vertex_only.replace(b"binary_little_endian", b"ascii") + face_head + b"end_header\n"
                                + b"0 0 0\n1 1 1\n-1 0 1\n",
        "ascii_count_above_uchar": vertex_only.replace(b"binary_little_endian", b"ascii") + face_head + b"end_header\n"
                                   + b"0 0 0\n1 1 1\n300 " + b"0 " * 300 + b"\n",
        "ascii_not_a_number": a.replace(b"end_header\n", b"end_header\nabc ", 1),
        "no_end_header": b[:hb - len(b"end_header\n")],
        "no_magic": b"plx\n" + b[4:],
        "no_format": b.replace(b"format binary_little_endian 1.0\n", b""),
        "unknown_type": b.replace(b"property float y", b"property half y"),
        "no_vertex_element": b"ply\nformat ascii 1.0\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n",
        "negative_element_count": b.replace(b"element vertex %d" % len(x), b"element vertex -1"),
        "empty_file": b"",
    }
    out = []
    for name, data in cases.items():
        p = os.path.join(d, f"bad_{name}.ply")
        with open(p, "wb") as f:
            f.write(data)
        out.append((name, p))
    out.append(("missing_file", os.path.join(d, "does_not_exist.ply")))
    return out
