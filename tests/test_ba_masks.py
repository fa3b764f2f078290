"""The row masks of the BA factorization plan (ba_plan.cpp row_masks / item_masks, host only), on camera
graphs that are not rings.

chol_factor (ba_chol.hpp) skips the matrix-core steps, W_k row loads and sweeps the masks declare
structurally zero.  A mask that drops a nonzero chunk removes a fill-in term from the Schur complement,
and LM still converges: the GPU suite's cost tolerance cannot see it.  Here the plan's schedule runs in
numpy twice on a random SPD system with the graph's block pattern: once without masks (what the
per-level launches chol_level do), once restating what chol_factor does with the uploaded per-item
words -- W_k rows present only in the loaded chunks and NaN elsewhere, the products over the range from
the lowest to the highest chunk of their mask and on the masked strips / column tiles only, padding
panels set instead of swept, the pre-sweep -- and the two must agree exactly.

Both executors accumulate a tile product as rank-1 terms in ascending k, so leaving out a term that is
an exact zero keeps every bit (up to the sign of a zero), as on the matrix cores."""
import numpy as np
import pytest

from sfmx import ba
from ba_graph_cases import HOLED, GRAPHS, ring, has_hole, hull, spd_system
from test_ba_plan import NB

NW = NB // 16
ORDERS = [ba.ORDER_AUTO, ba.ORDER_NATURAL, 2, 4]   # automatic, natural, nested dissection with leaves of 1 / 4 tiles
CASES = dict(GRAPHS, ring200=lambda: ring(200, 6), ring40=lambda: ring(40, 6),
             dense12=lambda: np.ones((12, 12), np.uint8) - np.eye(12, dtype=np.uint8))
assert NB == 64, "the row masks are 64-bit rows of 64-row tiles (ba_plan.cpp row_masks)"


class Poisoned(Exception):
    """A product read a W_k row that was not loaded (NaN)."""


_plans = {}


def plan_of(name, order):
    if (name, order) not in _plans:
        adj = CASES[name]()
        _plans[name, order] = (adj, ba.factor_plan(adj, order))
    return _plans[name, order]


def tile(i):
    return slice(i * NB, (i + 1) * NB)


def bits(m, n):
    return [q for q in range(n) if (int(m) >> q) & 1]


def expand(m, n, width):
    """Boolean vector of n * width entries: entry i is set when bit i // width of m is."""
    return np.repeat([(int(m) >> q) & 1 == 1 for q in range(n)], width)


def prod(A, Bt, ks):
    """sum over k in ks (ascending) of the rank-1 terms A[:, k] (x) Bt[:, k]."""
    acc = np.zeros((NB, NB))
    for k in ks:
        acc += np.multiply.outer(A[:, k], Bt[:, k])
    return acc


def chunk_range(m):
    """The k range the kernels multiply over for a chunk mask: lowest to highest set chunk (mfma_spread)."""
    h = hull(m)
    return [4 * q + i for q in bits(h, NB // 4) for i in range(4)]


def sweep(t, s):
    """One symmetric block sweep of the 16-row panel s (ba_chol.hpp diag_sweeps)."""
    B = slice(16 * s, 16 * s + 16)
    nb = np.ones(NB, bool)
    nb[B] = False
    Pc = t[:, B].copy()
    Q = np.linalg.inv(Pc[B])
    M = Pc @ Q
    t[np.ix_(nb, nb)] -= M[nb] @ Pc[nb].T
    t[B, nb] = Q @ Pc[nb].T
    t[nb, B] = M[nb]
    t[B, B] = -Q


def set_padding_panel(t, s):
    """What chol_factor does for an identity padding panel instead of sweeping it."""
    B = slice(16 * s, 16 * s + 16)
    t[:, B] = 0.0
    t[B, B] = -np.eye(16)


def item_index(plan):
    """Per src entry its chol_factor item; the items come leaves first, then level by level in task order."""
    isrc = plan["item_src"]
    nl = len(plan["leaves"])
    order = [s for _, _, _, _, s0, s1 in plan["tasks"] for s in range(s0, s1)]
    assert list(isrc[:nl]) == [-1] * nl and list(isrc[nl:]) == order
    return {int(s): i for i, s in enumerate(isrc) if s >= 0}


def execute(plan, S, b, masked, load=None, observe=None):
    """The plan's schedule in numpy.  masked: restate chol_factor with the per-item words plan["item_mask"]
    (load: per item the chunk mask of the W_k rows present, default the uploaded y); else the unmasked
    per-level form.  observe(s, a, bb, A_ak, A_bk) is called per (task, source) before its update.
    -> (A, W, U, x): the final lower tiles, the inverses, the upper tiles G^T, the solution."""
    T = plan["tiles"]
    im = plan["item_mask"]
    it_of = item_index(plan)
    nl = len(plan["leaves"])
    A, r = S.copy(), b.copy()
    W, U = {}, {}
    full = (1 << NW) - 1

    def invert(t, a, done, pad):
        for s in range(NW):
            if (done >> s) & 1:
                continue
            if (pad >> s) & 1:
                set_padding_panel(t, s)
            else:
                sweep(t, s)
        W[a] = -t
        r[tile(a)] = W[a] @ r[tile(a)]

    for i, k in enumerate(plan["leaves"]):
        invert(A[tile(k), tile(k)].copy(), int(k), 0, (im[i, 0] >> 12) & 15 if masked else 0)
    assert nl == len(W)
    tasks, src = plan["tasks"], plan["src"]
    for _, a, bb, inv, s0, s1 in tasks:
        a, bb = int(a), int(bb)
        diag = a == bb
        t = A[tile(a), tile(bb)].copy()
        x0 = int(im[it_of[s0], 0])
        pre = (x0 >> 16) & 15   # the same pre-sweep in every factorization form
        assert pre == 0 or (inv and diag and s1 - s0 == 1)
        for s in bits(pre, NW):
            sweep(t, s)
        for s in range(s0, s1):
            k = int(src[s])
            Aak, Abk = A[tile(a), tile(k)], A[tile(bb), tile(k)]
            if observe:
                observe(s, a, bb, Aak, Abk)
            if masked:
                x, y, z, _ = (int(v) for v in im[it_of[s]])
                ld = y if load is None else int(load[it_of[s]])
                Wk = np.where(expand(ld, NB // 4, 4)[:, None], W[k], np.nan)   # the rows tile_load_wt_rows writes
                ra, rb, gc = expand(x & 15, NW, 16), expand((x >> 4) & 15, NW, 16), expand((x >> 8) & 15, NW, 16)
                G = np.where(np.outer(ra, gc), prod(Aak, Wk.T, chunk_range(ld)), 0.0)   # spread_store's zeros
                Uab = np.where(np.outer(ra, rb), prod(G, Abk, chunk_range(z)), 0.0)
                if np.isnan(G).any() or np.isnan(Uab).any():
                    raise Poisoned(f"task ({a}, {bb}) source {k}")
            else:
                G = prod(Aak, W[k].T, range(NB))
                Uab = prod(G, Abk, range(NB))
            t -= Uab
            if diag:
                r[tile(a)] -= Aak @ r[tile(k)]
                U[k, a] = G.T
        if inv:
            assert diag
            invert(t, a, pre, (x0 >> 12) & 15 if masked else 0)
        else:
            A[tile(a), tile(bb)] = t
    assert set(W) == set(range(T))
    for k in range(T - 1, -1, -1):   # back solve in index order
        for (kk, a), u in U.items():
            if kk == k:
                r[tile(k)] -= u @ r[tile(a)]
    return A, W, U, r


def raw_ka(plan):
    """Per item the unfilled ka of its src entry (what chol_factor loaded before the hull fill)."""
    return np.array([plan["src_mask"][s, 2] if s >= 0 else 0 for s in plan["item_src"]])


def same_masks(p, q):
    return all(np.array_equal(p[k], q[k]) for k in ("camrow", "leaves", "tasks", "src", "src_mask", "pad_panels",
                                                    "item_mask", "item_src"))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_masks_cover_the_nonzeros(name, order):
    """Superset: in the unmasked execution every nonzero of A_ak / A_bk lies inside its strips and chunks,
    G's column tiles cover what G A_bk^T reads, and the padding panels are exactly the camera-free ones."""
    adj, plan = plan_of(name, order)
    S, b, pad = spd_system(adj, plan, seed=1)
    sm, im, it_of = plan["src_mask"], plan["item_mask"], item_index(plan)
    seen = []

    def observe(s, a, bb, Aak, Abk):
        ra, rb, ka, kb = (int(v) for v in sm[s])
        for M, rows, cols, tag in ((Aak, ra, ka, "A_ak"), (Abk, rb, kb, "A_bk")):
            nzr, nzc = (M != 0).any(1), (M != 0).any(0)
            assert not (nzr & ~expand(rows, NW, 16)).any(), (tag, "rows", s, a, bb)
            assert not (nzc & ~expand(cols, NB // 4, 4)).any(), (tag, "columns", s, a, bb)
        x, y, z, w = (int(v) for v in im[it_of[s]])
        assert (x & 15, (x >> 4) & 15, z, w) == (ra, rb, kb, 0)
        gc = (x >> 8) & 15
        if a == bb:
            assert gc == (1 << NW) - 1   # G^T is stored whole for the back solve
        else:
            assert not ((Abk != 0).any(0) & ~expand(gc, NW, 16)).any(), ("gc", s, a, bb)
        assert (y & ka) == ka and hull(y) == y, "the loaded W_k chunks cover the whole multiplied range"
        seen.append(s)

    A, W, U, x = execute(plan, S, b, masked=False, observe=observe)
    assert sorted(seen) == list(range(len(plan["src"])))
    x_ref = np.linalg.solve(S, b)
    assert np.max(np.abs(x - x_ref)) <= 1e-9 * np.max(np.abs(x_ref))   # (the pre-sweep order included)
    has_cam = ~pad
    want = [sum((0 if has_cam[a * NB + 16 * q: a * NB + 16 * q + 16].any() else 1) << q for q in range(NW))
            for a in range(plan["tiles"])]
    covered = np.zeros(plan["npad"], bool)
    for r0 in plan["camrow"]:
        covered[r0:r0 + 6] = True
    assert np.array_equal(covered, has_cam)
    assert list(plan["pad_panels"]) == want
    for i, k in enumerate(plan["leaves"]):
        assert tuple(im[i]) == (want[k] << 12, 0, 0, 0)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_masked_execution_equals_unmasked(name, order):
    adj, plan = plan_of(name, order)
    S, b, _ = spd_system(adj, plan, seed=2)
    A0, W0, U0, x0 = execute(plan, S, b, masked=False)
    A1, W1, U1, x1 = execute(plan, S, b, masked=True)
    for v in (A0, x0, A1, x1, *W0.values(), *W1.values(), *U0.values(), *U1.values()):
        assert not np.isnan(v).any()
    assert np.array_equal(x0, x1)
    assert np.array_equal(np.tril(A0), np.tril(A1))
    assert W0.keys() == W1.keys() and all(np.array_equal(W0[k], W1[k]) for k in W0)
    assert U0.keys() == U1.keys() and all(np.array_equal(U0[k], U1[k]) for k in U0)


@pytest.mark.parametrize("name", sorted(HOLED))
def test_holed_masks_poison_the_unfilled_load_and_not_the_uploaded_one(name):
    """The hazard: with the raw ka as the load mask (the kernel before the hull fill) a product meets a
    W_k row that was never loaded; with the uploaded y it does not."""
    adj, plan = plan_of(name, ba.ORDER_AUTO)
    assert any(has_hole(ka) for ka in plan["src_mask"][:, 2]), "no holed ka: replace this graph"
    S, b, _ = spd_system(adj, plan, seed=3)
    with pytest.raises(Poisoned):
        execute(plan, S, b, masked=True, load=raw_ka(plan))
    execute(plan, S, b, masked=True)
    assert all(hull(y) == int(y) for y in plan["item_mask"][:, 1])


def test_c5_ring_has_no_holed_mask():
    """The benchmark's graph: the hull fill changes no word chol_factor reads there."""
    _, plan = plan_of("ring200", ba.ORDER_AUTO)
    assert not any(has_hole(ka) for ka in plan["src_mask"][:, 2])
    assert np.array_equal(plan["item_mask"][:, 1], raw_ka(plan))


@pytest.mark.parametrize("name", sorted(CASES))
def test_masks_of_one_triangle_equal_those_of_the_symmetric_graph(name):
    for order in ORDERS:
        adj, plan = plan_of(name, order)
        assert same_masks(ba.factor_plan(np.triu(adj), order), plan), ("upper", order)
        assert same_masks(ba.factor_plan(np.tril(adj), order), plan), ("lower", order)
