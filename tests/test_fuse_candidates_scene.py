"""tests/fuse_points_scene.py: the numpy restatement of vpFuseCandidates against the plain loop of LocalMapping.cc:826-846 on random lists
with duplicates inside a list and across lists, -1 entries and bad points."""
import numpy as np
import pytest

import fuse_points_scene as fps


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_the_loop(seed):
    rng = np.random.default_rng(500 + seed)
    cap = int(rng.integers(20, 400))
    bad = rng.random(cap) < 0.2
    lists = []
    for _ in range(int(rng.integers(1, 6))):
        a = rng.integers(0, cap, int(rng.integers(0, 300))).astype(np.int32)
        a[rng.random(len(a)) < 0.3] = -1
        if len(a) > 4:
            a[-1] = a[0]                                         # a duplicate inside the list
            if lists and len(lists[0]):
                a[1] = lists[0][0]                               # and across lists
        lists.append(a)
    flat = np.concatenate(lists)
    named = flat[flat >= 0]
    assert len(named) > len(np.unique(named)) or len(named) < 2  # duplicates are there
    assert bad[named].any() or len(named) < 5
    want = fps.candidates_loop(lists, bad)
    got = fps.candidates(lists, bad)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert len(np.unique(got)) == len(got) and not bad[got].any()


def test_edges():
    bad = np.array([0, 1, 0], bool)
    assert len(fps.candidates([], bad)) == 0 and len(fps.candidates_loop([], bad)) == 0
    assert len(fps.candidates([np.full(5, -1)], bad)) == 0
    assert len(fps.candidates([[1, 1, -1]], bad)) == 0           # all bad
    assert np.array_equal(fps.candidates([[2, 1, 0], [0, 2]], bad), [2, 0])
    assert np.array_equal(fps.candidates_loop([[2, 1, 0], [0, 2]], bad), [2, 0])
