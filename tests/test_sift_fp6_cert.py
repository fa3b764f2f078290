"""CPU: the one-subset certificate of the FP6 SIFT screen (csrc/sift_fp6.hpp, fp6::certified).

tests/sift_fp6_cert_ref.py restates the certificate from its definition.  The header, compiled for the host
(tests/cpp/sift_fp6_cert_main.cpp, its own main), must agree with it bit for bit; every query the restatement
certifies must, by brute force over the exact distances, have its best row in subset r1 strictly ahead of
every row outside it, an exact s2 below 2^22, and the decision `a2 >= 2^22 or Lowe(a1, a2)` on the exact top-2
(a1, a2) of subset r1 alone equal to Lowe's test on the exact (s1, s2); and on the bench-like data nearly
every forwarded query must be certified.
Fails without the feature: the header has no fp6::certified."""
import os
import subprocess

import numpy as np
import pytest

import sift_fp6_cert_ref as cert
import sift_fp6_ref as ref
from sfmx import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = [0.7, 1.0, 1.5]
NAMES = ["synth", "uniform", "extreme", "midpoints"]


@pytest.fixture(scope="module")
def cases():
    return ref.cases()


@pytest.fixture(scope="module")
def screens(cases):
    return {(name, ratio): cert.screen(*cases[name], ratio) for name in NAMES for ratio in RATIOS}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sift_fp6_cert") / "sift_fp6_cert_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    os.path.join(REPO, "tests", "cpp", "sift_fp6_cert_main.cpp"), "-o", str(exe)], check=True)
    return exe


REC = np.dtype([("k1", "<f4"), ("k2", "<f4"), ("r1", "<i4"), ("nt", "<i4"), ("na", "<i4"), ("e2q", "<i4"),
                ("emax2", "<i4"), ("amax2", "<i4"), ("ratio", "<f8")])


def test_header_equals_the_restatement(driver, tmp_path, cases, screens):
    recs, exp = [], []
    for (name, ratio), s in screens.items():
        nt = len(cases[name][1])
        for nt_claimed in (nt, 1, 17):          # (the row count decides `usable` and r1 + 16 < nt)
            rec = np.zeros(len(s["k1"]), REC)
            rec["k1"] = s["k1"]
            rec["k2"] = np.where(s["usable"], s["k2"], ref.PAD_KEY)   # what the kernel holds where no second subset has a row
            rec["r1"], rec["nt"], rec["na"], rec["e2q"] = s["r1"], nt_claimed, s["na"], s["e2q"]
            rec["emax2"], rec["amax2"], rec["ratio"] = s["emax2"], s["amax2"], ratio
            recs.append(rec)
            exp.append(cert.certified(s["k1"], s["k2"], s["r1"], s["usable"] & (nt_claimed >= 2), nt_claimed, s["na"],
                                      s["e2q"], s["emax2"], s["amax2"], ratio))
    recs, exp = np.concatenate(recs), np.concatenate(exp)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([len(recs)], np.int32).tofile(f)
        recs.tofile(f)
    subprocess.run([str(driver), str(fin), str(fout)], check=True)
    got = np.fromfile(fout, np.int32)
    assert len(got) == len(exp) and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), exp)
    assert 0 < exp.sum() < len(exp)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("name", NAMES)
def test_certified_queries_are_settled_by_their_subset(cases, screens, name, ratio):
    q, t = cases[name]
    s = screens[(name, ratio)]
    assert not (s["certified"] & ~s["forward"]).any()
    idx = np.nonzero(s["certified"])[0]
    print(f"{name} ratio {ratio}: forwarded {int(s['forward'].sum())}, certified {len(idx)}")
    if len(idx) == 0:
        return
    S = cert.exact_s(q[idx], t)
    r1 = s["r1"][idx]
    inside = (np.arange(len(t))[None, :] % 16) == r1[:, None]
    big = np.iinfo(np.int64).max
    s_in = np.sort(np.where(inside, S, big), axis=1)
    a1, a2 = s_in[:, 0], s_in[:, 1]
    assert (a2 < big).all(), "a certified subset with fewer than two rows"
    s_out = np.where(inside, big, S).min(axis=1)
    assert (a1 < s_out).all(), "the best row is not strictly ahead of every row outside subset r1"
    s_all = np.sort(S, axis=1)
    s1, s2 = s_all[:, 0], s_all[:, 1]
    assert np.array_equal(s1, a1)
    assert (s2 < cert.SQRT_SAFE).all()
    decided = (a2 >= cert.SQRT_SAFE) | cert.lowe(a1, a2, ratio)
    assert np.array_equal(decided, cert.lowe(s1, s2, ratio))


def test_uniform_data_certifies_nothing(screens):
    for ratio in RATIOS:
        assert not screens[("uniform", ratio)]["certified"].any()


@pytest.fixture(scope="module")
def bench_like():
    return synth.sift_images(3, 8192)


@pytest.mark.parametrize("qi,ti", [(0, 1), (1, 2)])
def test_not_vacuous_on_bench_like_data(bench_like, qi, ti):
    """Rows [:2048] of one image against the whole next one at ratio 0.7: the certificate must cover at least
    95 % of the forwarded queries (the restatement gives 127 / 128 and 132 / 134)."""
    s = cert.screen(bench_like[qi][:2048], bench_like[ti], 0.7)
    fwd, c = int(s["forward"].sum()), int(s["certified"].sum())
    print(f"image {qi} -> {ti}: forwarded {fwd}, certified {c}")
    assert fwd >= 100
    assert c >= 0.95 * fwd
