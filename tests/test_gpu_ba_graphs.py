"""GPU: bundle adjustment on camera graphs that are not rings (tests/ba_graph_cases.py).

Every other BA problem of the suite gives each point consecutive cameras, and on such a banded graph no
row mask of the factorization (ba_plan.cpp row_masks) has a hole; chol_factor's masked products were only
ever compared with the unmasked per-level launches on one ring.  Here the solver's graph is the
prescribed one, its uploaded per-item masks are the host export (whose contract tests/test_ba_masks.py
checks without a GPU), the solve meets the oracle under the suite's tolerances, and three forms of the
same factorization agree bit for bit: the product library (chol_factor with the masks), the diagnostic
library with its W_k buffer filled with NaNs before the masked row load (SFMX_BA_POISON: a product over
a row that was not loaded then fails every time, whatever LDS held), and the diagnostic library's
unmasked per-level launches."""
import ctypes as C

import numpy as np
import pytest

from sfmx import ba
from ba_graph_cases import HOLED, has_hole, hull, problem
from diag import diagnostic
from test_gpu_ba import COST_RTOL

pytestmark = pytest.mark.gpu

POINTS = {"skip_ring": 2400, "hub_ring": 1500, "random": 1500, "chain_links": 1500, "two_clusters": 2400,
          "disconnected": 1500}
CASES = [(name, 3) for name in sorted(HOLED)] + [("skip_ring", 1), ("skip_ring", 7), ("two_clusters", 3),
                                                 ("disconnected", 3)]
FORM_ITERATIONS = 5


def run_form(p, **env):
    """5 LM iterations on a fresh context of the diagnostic library -> (result, items, masks)."""
    with diagnostic(**env) as dl:
        ctx = ba.BAContext(ba.BAProblem(**p), ba.default_options())
        try:
            sm, tr = ctx.run(max_iterations=FORM_ITERATIONS, trace_cap=64)
            P = ctx.get()
            n = dl.sfmx_ba_debug_chol_items(ctx._h, None, 0)
            assert n > 0
            buf = np.zeros(8 * n, np.int32)
            assert dl.sfmx_ba_debug_chol_items(ctx._h, buf.ctypes.data, len(buf)) == n
        finally:
            ctx.close()
    return (P.points.copy(), P.poses.copy(), P.intr.copy(), sm["final_cost"], tr.copy()), buf[:4 * n].reshape(n, 4), \
        buf[4 * n:].reshape(n, 4)


@pytest.mark.parametrize("name,model", CASES, ids=[f"{n}-k{m}" for n, m in CASES])
def test_non_ring_graph_matches_oracle_and_every_form_agrees(name, model):
    from oracle import oracle
    p, adj = problem(name, POINTS[name], seed=31, cam_model=model)
    nc = adj.shape[0]

    # the graph the solver derives is the prescribed one
    with diagnostic() as dl:
        got = np.zeros((nc, nc), np.uint8)
        assert dl.sfmx_ba_debug_adjacency(ba.BAProblem(**p).struct(), 0, got.ctypes.data_as(C.POINTER(C.c_uint8))) >= 0
    assert np.array_equal(got, adj)
    plan = ba.factor_plan(adj, ba.ORDER_AUTO)
    assert plan["tiles"] >= 3
    if name in HOLED:
        assert plan["height"] >= 2
        assert any(has_hole(ka) for ka in plan["src_mask"][:, 2]), "no holed ka: replace this graph"

    # the oracle, exactly as test_gpu_ba.test_solve_matches_oracle asks
    _, osm, otr = oracle.ba_solve(p, trace_cap=512)
    P = ba.BAProblem(**p)
    sm, tr = ba.solve(P, ba.default_options(), trace_cap=512)
    assert sm["termination_type"] == osm["termination_type"]
    assert abs(sm["initial_cost"] - osm["initial_cost"]) <= 1e-12 * osm["initial_cost"]
    assert abs(sm["final_cost"] - osm["final_cost"]) <= COST_RTOL * osm["final_cost"]
    n = min(len(tr), len(otr))
    assert np.array_equal(tr[:n, 2], otr[:n, 2])
    np.testing.assert_allclose(tr[:n, 0], otr[:n, 0], rtol=1e-6)

    # the product library's masked one-launch factorization ...
    P = ba.BAProblem(**p)
    sm, tr = ba.solve(P, ba.default_options(max_num_iterations=FORM_ITERATIONS), trace_cap=64)
    product = (P.points.copy(), P.poses.copy(), P.intr.copy(), sm["final_cost"], tr.copy())
    assert len(tr) >= 2 and np.isfinite(sm["final_cost"])
    # ... the same with every W_k row it does not load poisoned, and the unmasked per-level launches
    poisoned, items, masks = run_form(p, SFMX_BA_ORDER="auto", SFMX_BA_POISON="1")
    unmasked, items0, masks0 = run_form(p, SFMX_BA_ORDER="auto", SFMX_BA_POISON="0", SFMX_BA_BACK="0", SFMX_BA_SPLIT="0",
                                        SFMX_BA_DAG="0")

    # the uploaded per-item words are the host export for this graph and order
    for it, mk in ((items, masks), (items0, masks0)):
        assert np.array_equal(mk, plan["item_mask"])
        assert np.array_equal(it[:, 1], plan["item_src"])
        assert all(hull(y) == int(y) for y in mk[:, 1])
    if name in HOLED:
        raw = [plan["src_mask"][s, 2] for s in items[:, 1] if s >= 0]
        assert any(has_hole(ka) for ka in raw)

    for key, other in (("poisoned", poisoned), ("unmasked", unmasked)):
        assert product[3] == other[3], key
        for a, b in zip(product, other):
            assert np.array_equal(a, b), key
