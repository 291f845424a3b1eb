"""What the scenes of tests/bow_targets_scene.py contain, with the oracle alone (no GPU): the GPU tests of dvm_search_by_bow_targets
(tests/test_gpu_bow_targets.py) compare against oracle.search_by_bow_kf_kf on these scenes, so the scenes must really hold the cases
those tests are about.  walk() -- the Python restatement with the bookkeeping -- is pinned to the oracle first."""
import numpy as np
import pytest

import bow_targets_scene as bts


def _same(oracle, cur, tgt, nnratio, check_ori):
    n, idx, st = bts.walk(cur, tgt, nnratio, check_ori)
    want_n, want_ids = bts.oracle_row(oracle, cur, tgt, nnratio, check_ori)
    assert n == want_n and np.array_equal(bts.ids_of([tgt], idx[None])[0], want_ids)
    return n, idx, st


@pytest.mark.parametrize("dup", [0.0, 0.3])
@pytest.mark.parametrize("T", [1, 3, 11])
def test_grid_scenes(oracle, T, dup):
    sc = bts.scene(0, T, dup=dup)
    cur = sc["cur"]
    assert 300 <= len(cur["desc"]) <= 400 and 30 <= len(cur["fv"]["fv_nodes"]) <= 40       # (a vocabulary of 40 nodes)
    for tgt in sc["targets"]:
        assert 300 <= len(tgt["desc"]) <= 400 and 30 <= len(tgt["fv"]["fv_nodes"]) <= 40
        assert 0.4 <= (tgt["mp"] >= 0).mean() <= 0.6 and tgt["bad"].sum() >= 3                 # about half mapped, some of them bad
        assert len(np.unique(tgt["mp"][tgt["mp"] >= 0])) == (tgt["mp"] >= 0).sum()              # ids unique inside a keyframe
        for nnratio in (0.6, 0.9):
            for check_ori in (True, False):
                n, idx, st = _same(oracle, cur, tgt, nnratio, check_ori)
                assert st["max_usable"] > 64                                                    # a node the lanes scan in more than one step
                if dup:
                    assert st["claim_mattered"] >= 1                                            # a query whose result the earlier claims decide
        n_ori, n_all = _same(oracle, cur, tgt, 0.9, True)[0], _same(oracle, cur, tgt, 0.9, False)[0]
        assert 40 <= n_ori < n_all                                                              # the rotation check takes matches back


def test_ratio_matters_with_duplicates(oracle):
    sc = bts.scene(0, 3, dup=0.3)
    for tgt in sc["targets"]:
        assert bts.oracle_row(oracle, sc["cur"], tgt, 0.6, False)[0] < bts.oracle_row(oracle, sc["cur"], tgt, 0.9, False)[0]


@pytest.mark.parametrize("k", [63, 64, 65, 129])
def test_edge_scenes(oracle, k):
    sc = bts.edge_scene(k)
    tgt = sc["targets"][0]
    fv = tgt["fv"]
    assert list(fv["fv_nodes"]) == [4, 10, 20]
    in_node = fv["fv_feat"][fv["fv_off"][1]:fv["fv_off"][2]]
    assert bts.usable(tgt)[in_node].sum() == k and len(in_node) > k and bts.usable(tgt)[in_node[-1]]
    n, idx, st = _same(oracle, sc["cur"], tgt, 0.9, False)
    assert st["max_usable"] == k and n >= 20 and in_node[-1] in idx


def test_boundary_scene(oracle):
    sc = bts.boundary_scene()
    for tgt in sc["targets"]:
        for check_ori in (True, False):
            n, idx, st = _same(oracle, sc["cur"], tgt, 0.9, check_ori)
            assert st["best"][0] == (50, 128) and st["best"][1] == (49, 128)
            assert idx[0] == -1 and tgt["mp"][idx[1]] == 11
            n_le, idx_le, _ = bts.walk(sc["cur"], tgt, 0.9, check_ori, th_low_inclusive=True)     # what <= would give: one match more
            assert tgt["mp"][idx_le[0]] == 10 and n_le == n + 1


def test_nodes_are_independent(oracle):
    """The common nodes walked in reversed order (every id n replaced by 10000 - n in both keyframes, which reverses the ascending walk
    and keeps each node's lists) leave the oracle's result unchanged: the claims of one node never reach another."""
    for dup in (0.0, 0.3):
        sc = bts.scene(0, 3, dup=dup)
        rev = lambda n: 10000 - n                                                                  # noqa: E731
        cur_r = bts.renoded(sc["cur"], rev)
        assert np.array_equal(cur_r["fv"]["fv_nodes"], (10000 - sc["cur"]["fv"]["fv_nodes"])[::-1])
        for tgt in sc["targets"]:
            for nnratio, check_ori in ((0.9, True), (0.6, False)):
                a = bts.oracle_row(oracle, sc["cur"], tgt, nnratio, check_ori)
                b = bts.oracle_row(oracle, cur_r, bts.renoded(tgt, rev), nnratio, check_ori)
                assert a[0] == b[0] > 40 and np.array_equal(a[1], b[1])


def test_full_size_scene(oracle):
    sc = bts.scene(2, 33, n_pts=1000, n_clutter=250, n_nodes=300, dup=0.1, heavy_frac=0.1)
    assert len(sc["targets"]) == 33 and all(1100 <= len(k["desc"]) <= 1200 for k in [sc["cur"]] + sc["targets"])
    assert bts.oracle_row(oracle, sc["cur"], sc["targets"][32])[0] > 150
