"""A route change between runs of one matcher replans (diagnostic library).

The run plan of a matcher (pair order, work items, the per-pair records of the list path, the batches) is reused
while the pair list, the images and the run's route are those of the last run.  One matcher is run repeatedly with
only the tuning variables changing between runs: list path <-> dense arrays, FP6 <-> int8 screens, one batch <->
overlapped batches, persistent screens; every run must give the oracle's arrays byte for byte.  A value the
diagnostic library does not know fails the run with SFMX_EINVAL (the Python wrapper raises that code as a
ValueError carrying the SfmxError text) and names the variable and the value; the matcher stays usable."""
import contextlib
import os

import numpy as np
import pytest

import sfmx
from sfmx import _lib, synth
from diag import diagnostic

pytestmark = pytest.mark.gpu

ROUTE_VARS = ("SFMX_SIFT_VARIANT", "SFMX_SIFT_P2", "SFMX_ORB_VARIANT", "SFMX_MATCH_BATCHES", "SFMX_SCREEN_PERSIST")


@contextlib.contextmanager
def route_env(env):
    """Exactly the given route variables for the block; the caller's values come back afterwards."""
    saved = {k: os.environ.pop(k, None) for k in ROUTE_VARS}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        yield
    finally:
        for k in ROUTE_VARS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def assert_same(got, off, exp, exp_off, what):
    assert np.array_equal(off, exp_off), (what, off, exp_off)
    assert got.tobytes() == exp.tobytes(), what


SIFT_SEQUENCE = [{}, {"SFMX_SIFT_VARIANT": 110}, {"SFMX_SIFT_VARIANT": 100}, {"SFMX_MATCH_BATCHES": 2},
                 {"SFMX_SIFT_VARIANT": 103, "SFMX_SIFT_P2": 0}, {}, {"SFMX_SIFT_VARIANT": 111},
                 {"SFMX_SIFT_VARIANT": 113}, {"SFMX_SCREEN_PERSIST": 1}, {}]
ORB_SEQUENCE = [{}, {"SFMX_ORB_VARIANT": 12}, {"SFMX_MATCH_BATCHES": 3}, {}]


def sift_case():
    base = synth.sift_images(5, 1100, seed=57)
    imgs = [b[:n] for b, n in zip(base, [1, 33, 513, 1100, 1100])]
    imgs.append(np.random.default_rng(59).random((300, 128), dtype=np.float32) * 40)   # not integral: fp32 pairs
    return sfmx.NORM_L2, imgs, SIFT_SEQUENCE, {"SFMX_SIFT_VARIANT": 20}


def orb_case():
    base = synth.orb_images(4, 1200, seed=61)
    imgs = [b[:n] for b, n in zip(base, [1200, 1, 700, 513])]
    return sfmx.NORM_HAMMING, imgs, ORB_SEQUENCE, {"SFMX_ORB_VARIANT": 6}


@pytest.mark.parametrize("case", [sift_case, orb_case], ids=["sift", "orb"])
def test_route_change_between_runs_replans(case):
    from oracle import oracle
    norm, imgs, sequence, unknown = case()
    pairs = sfmx.pairs_unordered(len(imgs))
    em, eoff = oracle.match_pairs(imgs, pairs, 0.7)
    with diagnostic(), route_env({}):
        m = sfmx.BFMatcher(norm)
        try:
            m.set_images(imgs)
            for step, env in enumerate(sequence):
                with route_env(env):
                    m.run(pairs, 0.7)
                    got, off, _ = m.fetch()
                assert_same(got, off, em, eoff, (step, env))
            # a value this library does not know: the run fails and says which, and the matcher stays usable
            (var, value), = unknown.items()
            with route_env(unknown), pytest.raises((_lib.SfmxError, ValueError)) as err:
                m.run(pairs, 0.7)
            assert "SFMX_EINVAL" in str(err.value) or getattr(err.value, "code", None) == _lib.SFMX_EINVAL
            assert f"{var}={value}" in str(err.value)
            m.run(pairs, 0.7)
            got, off, _ = m.fetch()
            assert_same(got, off, em, eoff, "after the unknown value")
        finally:
            m.close()
