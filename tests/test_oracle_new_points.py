"""Pins the scenes of tests/test_gpu_new_points.py with the oracle alone, so that the GPU parity tests cannot pass vacuously: enough
accepted points, neighbours the baseline test skips (decided far from the threshold), a LIVE sequential dependency between the
neighbours, and two records of one neighbour naming one KF2 keypoint.  The scenes with 5 and 30 neighbours must show all of it; with one
neighbour there is no later neighbour, so only what one neighbour can show is asked of it."""
import numpy as np
import pytest

import new_points_scene as nps

SEEDS = (0, 1)                       # the seeds of the GPU tests
PARAMS = (dict(), dict(check_ori=True))


def _chains(seed, n, **kw):
    sc = nps.prefix(nps.scene(seed), n)
    return sc, nps.oracle_chain(sc, **kw), nps.oracle_chain(sc, update_table=False, **kw)


@pytest.mark.parametrize("kw", PARAMS, ids=("plain", "check_ori"))
@pytest.mark.parametrize("n", [5, 30])
@pytest.mark.parametrize("seed", SEEDS)
def test_scene_is_not_vacuous(seed, n, kw):
    sc, dep, ind = _chains(seed, n, **kw)
    off = dep["pair_off"]
    accepted = np.array([(dep["status"][off[j]:off[j + 1]] == 0).sum() for j in range(n)])
    assert (accepted >= 20).sum() >= 3, accepted
    # the baseline test: somebody is skipped, nobody is decided near the threshold
    assert (dep["nb_status"] == 1).sum() >= 1
    assert np.all(np.abs(dep["ratios"].astype(np.float64) - 0.01) > 1e-3 * 0.01), dep["ratios"]
    assert np.array_equal(dep["nb_status"] == 1, np.isin(np.arange(n), nps.TINY_BASELINE + (nps.NEGATIVE_DEPTH,)))
    # the sequential dependency is live: pairs of a later neighbour that exist only when the table is never updated
    ioff = ind["pair_off"]
    only_independent = 0
    for j in range(1, n):
        d = {tuple(p) for p in dep["pairs"][off[j]:off[j + 1]]}
        only_independent = max(only_independent, sum(1 for p in ind["pairs"][ioff[j]:ioff[j + 1]] if tuple(p) not in d))
    assert only_independent >= 20, only_independent
    assert np.any(dep["nb_matches"] != ind["nb_matches"])
    # one idx2 named by two records of one neighbour
    assert any(len(np.unique(dep["pairs"][off[j]:off[j + 1], 1])) < off[j + 1] - off[j] for j in range(n))
    # the bookkeeping of the composition itself
    for j in range(n):
        assert np.all(np.diff(dep["pairs"][off[j]:off[j + 1], 0]) > 0)              # vMatchedPairs: ascending idx1
    got = np.nonzero(dep["new_point"] >= 0)[0]
    assert np.all(sc["cur"]["mp"][got] < 0) and np.all(dep["status"][dep["new_point"][got]] == 0) and np.array_equal(dep["pairs"][dep["new_point"][got], 0], got)
    assert len(got) == (dep["status"] == 0).sum()                                    # a keypoint receives a point once


@pytest.mark.parametrize("seed", SEEDS)
def test_single_neighbour_scene(seed):
    sc, dep, ind = _chains(seed, 1)
    assert dep["nb_status"][0] == 0 and (dep["status"] == 0).sum() >= 20
    nps.assert_same(dep, ind)


@pytest.mark.parametrize("seed", SEEDS)
def test_special_neighbours(seed):
    sc = nps.scene(seed)
    dep = nps.oracle_chain(nps.prefix(sc, 30))
    off = dep["pair_off"]
    assert dep["nb_status"][nps.NO_SHARED_NODE] == 0 and dep["nb_matches"][nps.NO_SHARED_NODE] == 0    # runs, finds nothing
    j = nps.OTHER_PYRAMID
    assert len(sc["neighbours"][j]["scale_factors"]) == len(sc["cur"]["scale_factors"]) and sc["neighbours"][j]["scale_factors"][1] != sc["cur"]["scale_factors"][1]
    assert (dep["status"][off[j]:off[j + 1]] == 0).sum() >= 5
    # the variants the GPU tests run reject some, but not all
    far = nps.oracle_chain(nps.prefix(sc, 30), far_points=True, th_far=9.0)
    assert (far["status"] == 8).sum() >= 10 and (far["status"] == 0).sum() >= 50
    tight = nps.oracle_chain(nps.prefix(sc, 30), cos_parallax_max=0.9996)
    assert (tight["status"] == 1).sum() > (dep["status"] == 1).sum()
    coarse = nps.oracle_chain(nps.prefix(sc, 30), coarse=True)
    assert coarse["nb_matches"].sum() > dep["nb_matches"].sum()
