"""CPU: csrc/pose_math.hpp compiled for the host equals tests/pose_ref.py as bit patterns.

A small stand-alone program (tests/cpp/pose_math_main.cpp, its own main, g++ -O2 -ffp-contract=off) runs the
header's five-point solver, Sampson error, pose candidates and cheirality test on the cases' samples; the kernel
compiles the same functions for gfx950.  Fails without the feature: the header does not exist.
"""
import os
import subprocess

import numpy as np
import pytest

import pose_cases
import pose_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pose_math") / "pose_math_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    os.path.join(REPO, "tests", "cpp", "pose_math_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _samples():
    """Minimal samples: noise-free ones, the prepared correspondences of the cases' pairs (planar, rotation, NaN
    among them) under the restatement's own RNG stream, and degenerate ones."""
    out = [q for q in pose_cases.minimal_samples(40, seed=3)[0]]
    case = pose_cases.small_case()
    cams = [pose_ref.cam_params(K, d) for K, d in case["cameras"]]
    pts = {}
    for name in ("len6", "len65", "planar", "rotation", "repeated", "nan"):
        p = case["names"].index(name)
        L, R = case["pairs"][p]
        m = case["matches"][case["offsets"][p]:case["offsets"][p + 1]]
        P, _ = pose_ref.prepare(case["kps"][L][m["queryIdx"]], case["kps"][R][m["trainIdx"]],
                                cams[case["shot_camera"][L]], cams[case["shot_camera"][R]])
        pts[name] = P
        rng = pose_ref.Rng()
        for _ in range(12):
            out.append(P[pose_ref.get_subset(rng, len(P))] if name != "repeated" else P[:5])
    out.append(np.vstack([pts["nan"][5:6], pts["nan"][:4]]))          # a NaN correspondence in the sample
    out.append(np.zeros((5, 4)))
    out.append(np.full((5, 4), np.inf))
    return out, pts


def test_header_equals_the_restatement_bit_for_bit(driver, tmp_path):
    samples, pts = _samples()
    models = [pose_ref.five_point(q) for q in samples]
    assert sum(len(m) for m in models) > 200 and any(len(m) == 0 for m in models)
    Es = [E for m in models for E in m][:120]
    P = np.vstack([pts["len65"], pts["nan"], pts["planar"]])
    P = P[np.arange(len(Es)) % len(P)]
    cands = [pose_ref.candidates(E) for E in Es]
    samp = [np.concatenate([E, P[i]]) for i, E in enumerate(Es)]
    chk = [np.concatenate([c[i % 4], P[i]]) for i, c in enumerate(cands)]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([len(samples), len(samp), len(Es), len(chk)], np.int32).tofile(f)
        np.concatenate([np.ravel(s) for s in samples] + samp + [np.ravel(E) for E in Es] + chk).astype(np.float64).tofile(f)
    subprocess.run([str(driver), str(fin), str(fout)], check=True)
    got = np.fromfile(fout, np.float64)
    k = 0
    for i, m in enumerate(models):
        exp = np.zeros(91)
        exp[0] = len(m)
        exp[1:1 + 9 * len(m)] = np.ravel(m)
        assert got[k:k + 91].tobytes() == exp.tobytes(), f"five-point sample {i}"
        k += 91
    for i, E in enumerate(Es):
        e = np.float64(pose_ref.sampson_error(E, P[i:i + 1])[0])
        assert got[k:k + 1].tobytes() == np.array([e]).tobytes() or (np.isnan(e) and np.isnan(got[k])), f"sampson {i}"
        k += 1
    for i, c in enumerate(cands):
        assert got[k:k + 48].tobytes() == np.ravel(c).astype(np.float64).tobytes(), f"candidates {i}"
        k += 48
    n_true = 0
    for i, c in enumerate(cands):
        v = bool(pose_ref.cheirality(c[i % 4], P[i:i + 1, 0], P[i:i + 1, 1], P[i:i + 1, 2], P[i:i + 1, 3])[0])
        assert got[k] == float(v), f"cheirality {i}"
        n_true += v
        k += 1
    assert k == len(got) and 0 < n_true < len(cands)
