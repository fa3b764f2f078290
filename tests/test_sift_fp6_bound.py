"""CPU: the conservative FP6 screen of the SIFT matcher (csrc/sift_fp6.hpp).

tests/sift_fp6_ref.py restates the quantiser, the packed row and the bound from the e2m3 format's
definition; the header, compiled for the host (tests/cpp/sift_fp6_main.cpp, its own main), must agree
with it value for value.  On every input the restatement must satisfy, for every query,
  * |key - quantised key| <= E for every train row, and
  * the exact int8 screen forwards  =>  the conservative screen forwards
(pass 2 is exact on whatever is forwarded, so the matcher's output is then unchanged).
Fails without the feature: the header does not exist."""
import os
import subprocess

import numpy as np
import pytest

import sift_fp6_ref as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return ref.cases()


@pytest.mark.parametrize("ratio", [0.7, 1.5])
@pytest.mark.parametrize("name", ["synth", "uniform", "extreme", "midpoints"])
def test_bound_holds_and_screen_is_conservative(cases, name, ratio):
    q, t = cases[name]
    c = ref.conservative(q, t, ratio)
    err = np.abs(c["kappa"] - c["kappa_q"]).max(axis=1)
    assert (err <= c["E"] + 1.0).all(), f"worst excess {(err - c['E']).max()}"   # (+1: one f32 rounding of acc, < 1 key unit)
    exact = ref.exact_forward(q, t, ratio)
    assert not (exact & ~c["forward"]).any(), "the conservative screen rejected a query the exact screen forwards"
    frac_exact, frac = exact.mean(), c["forward"].mean()
    print(f"{name} ratio {ratio}: exact screen forwards {frac_exact:.4f}, conservative {frac:.4f}, "
          f"median E {np.median(c['E']):.0f}, worst error {err.max():.0f}")
    if name == "synth" and ratio == 0.7:
        assert exact.any(), "vacuous: the exact screen forwards nothing"
        assert frac < 0.25
    if name == "uniform":
        # the only cap on uniform data: the restated arithmetic is exact (integers and halves in float64)
        assert (c["kappa"] * 2 == np.rint(c["kappa"] * 2)).all() and np.abs(c["kappa"]).max() < 2.0 ** 40


def test_quantiser_error_classes():
    u = np.arange(256)
    m, e = ref.quantise(u)
    a = u - ref.OFFSET
    assert (ref.SCALE * m + e == a).all()
    assert np.abs(m).max() <= 56 and set(np.abs(m)) <= set(ref.MAGS)        # nothing saturates
    assert (np.abs(e)[np.abs(a) < 64] <= 2).all() and (np.abs(e)[np.abs(a) < 128] <= 4).all() and np.abs(e).max() <= 8


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sift_fp6") / "sift_fp6_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    os.path.join(REPO, "tests", "cpp", "sift_fp6_main.cpp"), "-o", str(exe)], check=True)
    return exe


def test_header_equals_the_restatement(driver, tmp_path, cases):
    rows = np.concatenate([np.tile(np.arange(256, dtype=np.float32), 1).reshape(2, 128), ref.extreme_rows(), ref.midpoint_rows(),
                           cases["synth"][0][:64], cases["uniform"][0][:64]]).astype(np.uint8)
    recs = []
    for name, ratio in (("synth", 0.7), ("uniform", 0.7), ("extreme", 0.7), ("midpoints", 1.5), ("synth", 0.0), ("synth", -1.0)):
        c = ref.conservative(*cases[name], ratio)
        n = len(c["k1"])
        rec = np.zeros(n, np.dtype([("k1", "<f4"), ("k2", "<f4"), ("na", "<i4"), ("e2q", "<i4"), ("emax2", "<i4"),
                                    ("amax2", "<i4"), ("ratio", "<f8")]))
        rec["k1"], rec["k2"], rec["na"], rec["e2q"] = c["k1"], c["k2"], c["na"], c["e2q"]
        rec["emax2"], rec["amax2"], rec["ratio"] = c["emax2"], c["amax2"], ratio
        recs.append((rec, ref.certainly_rejected(c["k1"], c["k2"], c["na"], c["e2q"], c["emax2"], c["amax2"], ratio)))
    dec = np.concatenate([r for r, _ in recs])
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([len(rows), len(dec)], np.int32).tofile(f)
        rows.tofile(f)
        dec.tofile(f)
    subprocess.run([str(driver), str(fin), str(fout)], check=True)
    got = np.fromfile(fout, np.int32)
    per = got[:len(rows) * 154].reshape(len(rows), 154)
    m, e = ref.quantise(rows)
    assert np.array_equal(per[:, :128], m)
    assert np.array_equal(per[:, 128:152].view(np.uint32), ref.pack_rows(m))
    a = rows.astype(np.int64) - ref.OFFSET
    assert np.array_equal(per[:, 152], (a * a).sum(1))
    assert np.array_equal(per[:, 153], (e * e).sum(1))
    k = len(rows) * 154
    exp_rej = np.concatenate([r for _, r in recs])
    assert np.array_equal(got[k:k + len(dec)].astype(bool), exp_rej)
    assert 0 < exp_rej.sum() < len(exp_rej)
    k += len(dec)
    assert np.array_equal(got[k:k + 64], [ref.decode(c) for c in range(64)])


# Lane groups one LDS cycle serves (MI355X): ds_read_b128 in four groups of 16 lanes, ds_read_b64 in the two
# 32-lane halves; the bank of byte address a is (a / 4) mod 64 for both.
B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
               list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
B128_GROUPS += [[l + 32 for l in grp] for grp in B128_GROUPS]
B64_GROUPS = [list(range(0, 32)), list(range(32, 64))]


def test_lds_fragment_reads_are_conflict_free(driver, tmp_path):
    """sift_screen6_kernel's fragment reads (lane l: row l & 15, lane group g = l >> 4): the 16-B read of
    plane A (64-B rows, piece g at slot g ^ swz_a) and the 8-B read of plane B (32-B rows, piece g >> 1 at
    slot (g >> 1) ^ swz_b, half g & 1) touch every bank at most once per lane group.  The swizzles are the
    header's own (read back from the host program)."""
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        np.array([0, 0], np.int32).tofile(f)
    subprocess.run([str(driver), str(fin), str(fout)], check=True)
    swz = np.fromfile(fout, np.int32)[64:].reshape(16, 2)
    for row0 in (0, 16, 32, 112):           # the row blocks of a stage start at multiples of 16
        for groups, nbytes in ((B128_GROUPS, 16), (B64_GROUPS, 8)):
            for grp in groups:
                banks = []
                for l in grp:
                    row, g = row0 + (l & 15), l >> 4
                    if nbytes == 16:
                        a = row * 64 + 16 * (g ^ swz[row & 15, 0])
                    else:
                        a = row * 32 + 16 * ((g >> 1) ^ swz[row & 15, 1]) + 8 * (g & 1)
                    banks += [((a + 4 * k) // 4) % 64 for k in range(nbytes // 4)]
                assert len(set(banks)) == len(banks), (row0, nbytes, grp)
