"""CPU: the maps of the FP6 screen's 32 x 32 x 64 form (csrc/sift_fp6.hpp: frag32, acc_row32, chain_subset32 and
the LDS offsets lds_a32 / lds_b32 / lds_key32), printed by a host program of its own
(tests/cpp/sift_fp6_screen32_main.cpp).  sift_screen6w_kernel and its epilogue use the same functions.
Fails without the feature: the header has no such functions."""
import collections
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = 128
A_BYTES, B_BYTES = STAGE * 64, STAGE * 32


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sift_fp6_screen32") / "sift_fp6_screen32_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(REPO, "tests", "cpp", "sift_fp6_screen32_main.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    m = collections.defaultdict(dict)
    for line in out.splitlines():
        name, *v = line.split()
        v = [int(x) for x in v]
        m[name][tuple(v[:-1])] = v[-1]
    return m


def test_chain_to_subset_map(maps):
    chain, accrow = maps["chain"], maps["accrow"]
    assert len(chain) == 16 and len(accrow) == 32
    for c in range(8):
        for h in range(2):
            assert chain[c, h] == (c & 3) + 4 * h + 8 * (c >> 2)
    assert sorted(chain.values()) == list(range(16))                 # a bijection onto the 16 row subsets
    for h in range(2):
        assert sorted(accrow[i, h] for i in range(16)) == sorted(set(accrow[i, h] for i in range(16)))
        for i in range(16):
            assert accrow[i, h] == (i & 3) + 8 * (i >> 2) + 4 * h
        for c in range(8):                                           # registers c and c + 8 fold into chain c
            assert accrow[c, h] % 16 == accrow[c + 8, h] % 16 == chain[c, h]
            assert accrow[c + 8, h] == accrow[c, h] + 16
    assert sorted(accrow.values()) == list(range(32))                # the two halves cover the 32-row block


def test_fragment_map_is_a_bijection(maps):
    assert sorted(maps["frag"].values()) == [0, 1, 2, 3]


def test_reads_address_the_stage_layout(maps):
    """Every (row, fragment) has its own 16 B of plane A and its own 8 B of plane B, in the 16 x 16 form's layout
    (piece g at slot g ^ swz_a(row); piece g >> 1 at slot (g >> 1) ^ swz_b(row), half g & 1), and a lane's key
    reads are the keys of its accumulator rows."""
    a, b, key, accrow = maps["a"], maps["b"], maps["key"], maps["accrow"]
    assert len(a) == len(b) == 4 * STAGE
    assert sorted(a.values()) == list(range(0, A_BYTES, 16))
    assert sorted(b.values()) == list(range(A_BYTES, A_BYTES + B_BYTES, 8))
    for (row, f), off in a.items():
        assert off == row * 64 + 16 * (f ^ ((0 - (row >> 2)) & 3))
    for (row, f), off in b.items():
        assert off == A_BYTES + row * 32 + 16 * ((f >> 1) ^ ((row >> 3) & 1)) + 8 * (f & 1)
    for (row0, k, h), off in key.items():
        assert off == A_BYTES + B_BYTES + 4 * (row0 + accrow[4 * k, h])
        assert [accrow[4 * k + i, h] for i in range(4)] == [accrow[4 * k, h] + i for i in range(4)]


# Lane groups one LDS cycle serves (MI355X): ds_read_b128 in four groups of 16 lanes, ds_read_b64 in the two
# 32-lane halves; the bank of byte address a is (a / 4) mod 64 for both (tests/test_sift_fp6_bound.py).
B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
               list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
B128_GROUPS += [[l + 32 for l in grp] for grp in B128_GROUPS]
B64_GROUPS = [list(range(0, 32)), list(range(32, 64))]


def _bank_degree(addresses, nbytes):
    """The most distinct addresses (of nbytes each) that share a bank; lanes reading one address are a broadcast."""
    per_bank = collections.Counter()
    for a in set(addresses):
        for k in range(nbytes // 4):
            per_bank[((a + 4 * k) // 4) % 64] += 1
    return max(per_bank.values())


@pytest.mark.parametrize("row0", [0, 32, 64, 96])
def test_lds_banks_of_the_reads(maps, row0):
    """Lane l reads row row0 + (l & 31), fragment frag(m, l >> 5).  Plane A: conflict-free.  Plane B: exactly the
    2-way conflict the header states (the 32 lanes of a half read 64 words from 32 banks).  Keys: one address
    per lane group (broadcast)."""
    frag, a, b, key = maps["frag"], maps["a"], maps["b"], maps["key"]
    for m in range(2):
        for grp in B128_GROUPS:
            addrs = [a[row0 + (l & 31), frag[m, l >> 5]] for l in grp]
            assert len(set(addrs)) == 16 and _bank_degree(addrs, 16) == 1, (row0, m, grp)
        for grp in B64_GROUPS:
            addrs = [b[row0 + (l & 31), frag[m, l >> 5]] for l in grp]
            assert len(set(addrs)) == 32 and _bank_degree(addrs, 8) == 2, (row0, m, grp)
    for k in range(4):
        for grp in B128_GROUPS:
            addrs = [key[row0, k, l >> 5] for l in grp]
            assert len(set(addrs)) == 1 and _bank_degree(addrs, 16) == 1, (row0, k, grp)
