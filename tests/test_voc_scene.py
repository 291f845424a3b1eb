"""The DBoW2-shaped vocabulary scenes (tests/voc_scene.py) hold what they were made for, and the oracle's transform equals the numpy
restatement on them.  CPU only; the GPU side is tests/test_gpu_vocab_trees.py."""
import numpy as np
import pytest

import voc_scene as vs
from dvm_slam_amd import synth

KL = list(vs.TREES)


def levelsups(L):
    return (0, 1, 2, L, L + 2)


@pytest.mark.parametrize("k,L", KL)
def test_tree_shape(k, L):
    voc, feats, _ = vs.scene(k, L)
    assert set(voc) >= set(synth.vocabulary(k=3, L=1))
    n, off, ch = voc["n_nodes"], voc["child_off"], voc["children"]
    assert n < 1500 and feats.shape == (vs.N_FEATS, 32)
    fan = np.diff(off)
    parent = np.repeat(np.arange(n), fan)
    assert np.all(ch > parent), "a child before its parent"
    assert np.array_equal(ch, np.arange(1, n)), "not breadth-first: every node but the root listed once, in id order"
    assert np.all(np.diff(voc["level"][1:]) >= 0) and np.array_equal(voc["level"][ch], voc["level"][parent] + 1)
    assert voc["level"].max() == L and fan[fan > 0].min() == 1 and fan.max() <= k
    assert (fan == 1).sum() >= 1, "no single-child node"
    if k > 16:
        assert (fan > 16).sum() >= 1, "no node of more than 16 children"
    if k == 16:
        assert (fan == 16).sum() >= 1, "no node of exactly 16 children"
    leaves = np.flatnonzero(fan == 0)
    assert ((voc["level"][leaves] < L).sum() >= 1) and np.array_equal(voc["word_id"][leaves], np.arange(len(leaves)))
    assert np.all(voc["word_id"][fan > 0] == -1)
    assert 1 <= (voc["weight"][leaves] == 0).sum() <= len(leaves) // 10
    sib = [voc["desc"][ch[off[i]:off[i + 1]]] for i in range(n) if fan[i] > 1]
    assert sum(len(d) - len(np.unique(d, axis=0)) for d in sib) >= 5, "no siblings of equal descriptors"


@pytest.mark.parametrize("k,L", KL)
def test_scene_reaches_what_it_is_for(k, L):
    voc, feats, down = vs.scene(k, L)
    assert (down["depth"] < L).sum() >= 100, "features that end on a leaf above level L"
    w1 = vs.walk(voc, feats, 1, down)
    assert (w1["node"] == -1).sum() >= 100 and w1["fv_nodes"][-1] == -1 and max(w1["fv"]) == 0xFFFFFFFF
    assert np.all(w1["fv_nodes"][:-1] >= 0) and np.all(np.diff(w1["fv_nodes"].astype(np.uint32).astype(np.int64)) > 0)
    assert down["tie"].sum() >= 100, "features that meet a tie at the minimum"
    if (k, L) == (20, 3):
        assert down["late"].sum() >= 50, "winners at child position 16 or later"
    g = down["depth"].reshape(-1, 4)                   # a wave of k_vocab_transform holds four consecutive features
    assert (g.min(axis=1) != g.max(axis=1)).sum() >= 100, "groups of four features that reach unequal depths"
    # the first child wins a tie: a feature never reaches a node that repeats an elder sibling's descriptor
    off, ch = voc["child_off"], voc["children"]
    younger = np.zeros(voc["n_nodes"], bool)
    for i in range(voc["n_nodes"]):
        c = ch[off[i]:off[i + 1]]
        for j in range(1, len(c)):
            younger[c[j]] = (voc["desc"][c[:j]] == voc["desc"][c[j]]).all(axis=1).any()
    assert younger.sum() >= 5 and not younger[down["path"][down["path"] >= 0]].any()


@pytest.mark.parametrize("k,L", KL)
def test_oracle_transform_equals_walk(oracle, k, L):
    voc, feats, down = vs.scene(k, L)
    for levelsup in levelsups(L):
        w = vs.walk(voc, feats, levelsup, down)
        r = oracle.vocab_transform(voc, feats, levelsup)
        for key in ("word", "node", "weight", "bow_ids", "bow_vals", "fv_nodes", "fv_off", "fv_feat"):
            assert np.array_equal(w[key], r[key]), (levelsup, key)
        assert w["bow_vals"].dtype == np.float64 and len(w["bow_ids"]) > 10
        if levelsup >= L:
            assert np.all(w["node"] == 0)
        if levelsup == 0:
            assert np.array_equal(w["node"] == -1, down["depth"] < L)
