"""CPU: csrc/pnp_math.hpp compiled for the host equals tests/pnp_ref.py as bit patterns.

A small stand-alone program (tests/cpp/pnp_math_main.cpp, its own main, g++ -O2 -ffp-contract=off) runs the
header's EPnP on five points, its reprojection error and the refit's pieces (the planarity test and the DLT start
from the inliers' sums, Rodrigues both ways, one point's projection terms, undistortion to double, the 6 x 6
solve) on the samples below; the kernel compiles the same
functions for gfx950.  Fails without the feature: the header does not exist.
"""
import os
import subprocess

import numpy as np
import pytest

import pnp_cases
import pnp_ref
import tri_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pnp_math") / "pnp_math_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    os.path.join(REPO, "tests", "cpp", "pnp_math_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _samples():
    """(5 x 3 points, 5 x 2 normalised image points): noise-free ones, the cases' subsets under the restatement's
    own RNG stream (planar, noise, NaN sets among them), and degenerate ones."""
    X, uv, _, _ = pnp_cases.minimal_samples(60, seed=3)
    out = [(X[i], uv[i]) for i in range(len(X))]
    case = pnp_cases.small_case()
    cams = [tri_ref.cam_params(K, d) for K, d in case["cameras"]]
    for name in ("len6", "len65", "len257", "planar", "noise", "nan"):
        s = case["names"].index(name)
        a, b = case["offsets"][s], case["offsets"][s + 1]
        X32, pt = case["p3"][a:b].astype(F32), case["p2"][a:b].astype(F32)
        cam = cams[case["shot_camera"][case["set_shot"][s]]]
        rng = pnp_ref.Rng()
        for _ in range(10):
            idx = pnp_ref.get_subset(rng, len(X32))
            x, y = tri_ref.undistort(pt[idx], cam)
            out.append((X32[idx].astype(F64), np.stack([x, y], axis=1).astype(F64)))
    X0, uv0 = out[0]
    flat = X0.copy()
    flat[:, 2] = 1.5                                              # coplanar five
    out.append((flat, uv0))
    rep = X0.copy()
    rep[3] = rep[1]                                               # a repeated point
    u2 = uv0.copy()
    u2[3] = u2[1]
    out.append((rep, u2))
    out.append((np.tile(X0[:1], (5, 1)), np.tile(uv0[:1], (5, 1))))   # one point five times
    bad = X0.copy()
    bad[2, 1] = np.nan
    out.append((bad, uv0))
    bad = uv0.copy()
    bad[4, 0] = np.nan
    out.append((X0, bad))
    out.append((np.zeros((5, 3)), np.zeros((5, 2))))
    out.append((np.full((5, 3), np.inf), uv0))
    return out, case, cams


def test_header_equals_the_restatement_bit_for_bit(driver, tmp_path):
    samples, case, cams = _samples()
    exp = [pnp_ref.epnp5(X, uv, detail=True) for X, uv in samples]
    assert sum(e is not None for e in exp) > 80 and sum(e is None for e in exp) >= 3
    assert {e[1] for e in exp if e is not None} == {1, 2, 3}      # every approximation wins somewhere
    # reprojection errors: the models above on points of both cameras (one distorted), a NaN point among them
    errs = []
    poses = [e[0] for e in exp if e is not None][:60]
    for i, pose in enumerate(poses):
        s = case["names"].index("nan" if i % 3 == 0 else "len257")
        k = case["offsets"][s] + (7 * i) % 64
        cam = cams[i % 2]
        X32, pt = case["p3"][k:k + 1].astype(F32), case["p2"][k:k + 1].astype(F32)
        errs.append((pose, X32, pt, cam))
    # the refit's pieces (host libm on both sides): Rodrigues both ways, one point's 28 addends, undistort_d, solve6
    rng = np.random.default_rng(5)
    refits = []
    for i, (pose, X32, pt, cam) in enumerate(errs[:40]):
        if np.isnan(X32).any() or np.isnan(pt).any():
            continue
        rvec = [0.0, 0.0, 0.0] if i == 1 else (rng.standard_normal(3) * (1e-9 if i == 2 else 0.3)).tolist()
        refits.append(rvec + [pose[3], pose[7], pose[11]] + X32[0].astype(F64).tolist() + pt[0].astype(F64).tolist() +
                      [cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")])
    # the refit's start: the inliers' sums (fixed tree order) of every posed set of the cases, under the golden masks of
    # the three thresholds, and degenerate matrices
    golden = np.load(os.path.join(REPO, "tests", "golden", "pnp_small.npz"))
    starts = []
    for ti in range(len(pnp_cases.THRESHOLDS)):
        for sidx in np.flatnonzero(golden[f"t{ti}_refit_start"] >= 0):
            a, b = case["offsets"][sidx], case["offsets"][sidx + 1]
            starts.append(pnp_ref.inlier_sums(case["p3"][a:b].astype(F32), case["p2"][a:b].astype(F32),
                                              golden[f"t{ti}_mask"][a:b].astype(bool),
                                              cams[case["shot_camera"][case["set_shot"][sidx]]]))
    S0, L0 = starts[0]
    starts.append(([0.0] * 6, [0.0] * 78))
    starts.append(([np.nan] + S0[1:], [np.nan] * 78))
    starts.append((S0, L0[:5] + [np.nan] + L0[6:]))
    starts.append(([1.0, 0.0, 0.0, 1.0, 0.0, 1e-4], [-v for v in L0]))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([len(samples), len(errs), len(refits), len(starts)], np.int32).tofile(f)
        rows = [np.concatenate([np.ravel(X), np.ravel(uv)]) for X, uv in samples]
        rows += [np.concatenate([pose, X32[0].astype(F64), pt[0].astype(F64),
                                 [cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]])
                 for pose, X32, pt, cam in errs]
        rows += [np.asarray(r, F64) for r in refits]
        rows += [np.asarray(S + LL, F64) for S, LL in starts]
        np.concatenate(rows).astype(F64).tofile(f)
    subprocess.run([str(driver), str(fin), str(fout)], check=True)
    got = np.fromfile(fout, F64)
    k = 0
    for i, e in enumerate(exp):
        want = np.zeros(14) if e is None else np.concatenate([[e[1]], e[0], [e[2]]]).astype(F64)
        assert got[k:k + 14].tobytes() == want.tobytes(), f"EPnP sample {i}"
        k += 14
    n_nan = 0
    for i, (pose, X32, pt, cam) in enumerate(errs):
        e = F64(pnp_ref.reprojection_error(pose, X32, pt, cam)[0])
        assert got[k:k + 1].tobytes() == np.array([e]).tobytes() or (np.isnan(e) and np.isnan(got[k])), f"error {i}"
        n_nan += bool(np.isnan(e))
        k += 1
    assert 0 < n_nan < len(errs) and len(refits) > 20
    for i, r in enumerate(refits):
        cam = dict(zip(("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"), [F64(v) for v in r[11:]]))
        R, dR = pnp_ref.rodrigues(r[:3])
        M, pt = np.array([r[6:9]], F64), np.array([r[9:11]], F64)
        S = pnp_ref.residuals(r[:6], M, pt, np.ones(1, bool), cam)
        ux, uy = pnp_ref.undistort64(pt.astype(F32), cam)
        A = [[0.0] * 6 for _ in range(6)]
        j = 0
        for a in range(6):
            for b in range(a, 6):
                A[a][b] = A[b][a] = float(S[j])
                j += 1
        for a in range(6):
            A[a][a] = A[a][a] + 1.0
        x = pnp_ref.solve6(A, [float(v) for v in S[21:27]])
        want = np.concatenate([R, np.ravel(dR), pnp_ref.rodrigues_inv(R), S, [ux[0], uy[0]], x if x is not None else np.zeros(6)])
        g = got[k:k + 75]
        assert (g == want.astype(F64)).all(), (f"refit pieces {i}", np.flatnonzero(g != want))      # == : -0 is 0
        k += 75
    n_ok = n_planar = 0
    for i, (S, LL) in enumerate(starts):
        planar = pnp_ref.planar_cov(list(S))
        st = pnp_ref.dlt_start(list(LL))
        want = np.zeros(17)
        want[0] = float(planar)
        if st is not None:
            want[1] = 1.0
            want[2:11], want[11:14], want[14:17] = st[0], st[1], pnp_ref.rodrigues_inv(st[0])
        assert got[k:k + 17].tobytes() == want.tobytes(), (f"refit start {i}", got[k:k + 17], want)
        n_ok += st is not None
        n_planar += planar
        k += 17
    assert k == len(got) and n_ok >= 24 and 0 < n_planar < len(starts) and n_ok < len(starts)
