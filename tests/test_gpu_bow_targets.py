"""dvm_search_by_bow_targets (ORBmatcher::SearchByBoW(cur, target) for all the candidate and covisible keyframes of
LoopClosing::DetectCommonRegionsFromBoW as one chain) against oracle.search_by_bow_kf_kf on every target alone: the map-point ids through
targets[t].mp[match_idx2], and nmatches.  Kernel and oracle make the same integer decisions, so every comparison is exact.  The scenes
are pinned by tests/test_oracle_bow_targets.py (CPU)."""
import numpy as np
import pytest

import bow_targets_scene as bts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.BowTargets()
    h.reserve(500, 11, 11 * 500)
    yield h
    h.close()


def _check(oracle, chain, cur, targets, nnratio=0.9, check_ori=True):
    idx, nm = chain.search(cur, targets, nnratio, check_ori)
    want_ids, want_nm = bts.oracle_rows(oracle, cur, targets, nnratio, check_ori)
    assert idx.shape == want_ids.shape and np.array_equal(nm, want_nm)
    assert np.array_equal(bts.ids_of(targets, idx), want_ids)
    for t, tgt in enumerate(targets):                   # a target keypoint is matched once (vbMatched2), and only a usable one
        j = idx[t][idx[t] >= 0]
        assert len(np.unique(j)) == len(j) and np.all(bts.usable(tgt)[j])
    return idx.copy(), nm.copy()


@pytest.mark.parametrize("check_ori", [True, False], ids=("ori", "no_ori"))
@pytest.mark.parametrize("nnratio", [0.6, 0.9])
@pytest.mark.parametrize("dup", [0.0, 0.3])
@pytest.mark.parametrize("T", [1, 3, 11])
def test_parity_grid(oracle, chain, T, dup, nnratio, check_ori):
    sc = bts.scene(0, T, dup=dup)
    _, nm = _check(oracle, chain, sc["cur"], sc["targets"], nnratio, check_ori)
    assert nm.min() >= 40


@pytest.mark.parametrize("k", [63, 64, 65, 129])
def test_scan_length_edges(oracle, chain, k):
    sc = bts.edge_scene(k)
    idx, nm = _check(oracle, chain, sc["cur"], sc["targets"], 0.9, False)
    tgt = sc["targets"][0]
    last = tgt["fv"]["fv_feat"][tgt["fv"]["fv_off"][1 + 1] - 1]          # the last scan position of node 10 (the second node)
    assert tgt["fv"]["fv_nodes"][1] == 10 and last in idx[0] and nm[0] >= 20


def test_long_scan(oracle, capi):
    """More than 4096 features in one node: the second half of the per-lane claim mask."""
    rng = np.random.default_rng(9)
    n2, hits = 4300, np.array([0, 63, 64, 4095, 4096, 4097, 4159, 4160, 4299])
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    tgt = bts.make_kf(d2, np.full(n2, 7), np.arange(n2) + 10, np.zeros(n2, np.uint8), rng.uniform(0, 360, n2), rng)
    # every hit is asked for twice: the second query finds its candidate claimed
    c = np.concatenate([bts.flip(rng, d2[hits], 5), bts.flip(rng, d2[hits], 7)])
    cur = bts.make_kf(c, np.full(len(c), 7), np.arange(len(c)) + 10, np.zeros(len(c), np.uint8), rng.uniform(0, 360, len(c)), rng)
    h = capi.BowTargets()
    h.reserve(len(c), 1, n2)
    idx, nm = _check(oracle, h, cur, [tgt], 0.9, False)
    h.close()
    assert np.array_equal(idx[0][:len(hits)], hits) and np.all(idx[0][len(hits):] == -1) and nm[0] == len(hits)


@pytest.mark.parametrize("check_ori", [True, False], ids=("ori", "no_ori"))
def test_strict_threshold(oracle, chain, check_ori):
    """best == 50 stays unmatched (ORBmatcher.cc:785 is <, where the KeyFrame -> Frame form has <=), best == 49 matches."""
    sc = bts.boundary_scene()
    idx, _ = _check(oracle, chain, sc["cur"], sc["targets"], 0.9, check_ori)
    for t, tgt in enumerate(sc["targets"]):
        assert idx[t][0] == -1
        assert idx[t][1] >= 0 and tgt["mp"][idx[t][1]] == 11       # the candidate 49 bits away


def test_degenerate_inputs(oracle, chain):
    sc = bts.scene(0, 3, dup=0.3)
    cur, tg = sc["cur"], sc["targets"]
    idx, nm = chain.search(bts.without_map_points(cur), tg)                # cur without map points
    assert np.all(idx == -1) and np.all(nm == 0)
    idx, nm = _check(oracle, chain, cur, [tg[0], bts.empty_kf(), tg[1]])  # a target with n = 0
    assert np.all(idx[1] == -1) and nm[1] == 0 and nm[0] > 40 and nm[2] > 40
    idx, nm = _check(oracle, chain, cur, [bts.renoded(tg[0], lambda n: n + 1), tg[1]])   # disjoint nodes
    assert np.all(idx[0] == -1) and nm[0] == 0 and nm[1] > 40
    idx, nm = _check(oracle, chain, cur, [tg[0], bts.all_bad(tg[1])])      # every mapped point of a target bad
    assert np.all(idx[1] == -1) and nm[1] == 0
    idx, nm = chain.search(cur, [])                                        # n_targets = 0
    assert idx.shape == (0, len(cur["desc"])) and nm.shape == (0,)
    idx, nm = chain.search(bts.empty_kf(), tg)                             # cur->n = 0
    assert idx.shape == (3, 0) and np.all(nm == 0)
    one = [bts.renoded(k, 5) for k in [cur] + tg]                          # all features in one node
    idx, nm = _check(oracle, chain, one[0], one[1:])
    assert nm.min() > 20
    neg = [bts.renoded(k, lambda n: np.where(n == 3, -1, n)) for k in [cur] + tg]   # node id -1 sorts last (unsigned)
    _check(oracle, chain, neg[0], neg[1:])
    few = bts.drop_features(cur, np.arange(0, len(cur["desc"]), 3))        # keypoints that no node lists
    idx, nm = _check(oracle, chain, few, tg)
    assert np.all(idx[:, ::3] == -1)


def test_rows_are_independent(oracle, chain):
    sc = bts.scene(0, 11, dup=0.3)
    cur, tg = sc["cur"], sc["targets"]
    idx, nm = chain.search(cur, tg)
    idx, nm = idx.copy(), nm.copy()
    for t in range(11):
        i1, n1 = chain.search(cur, [tg[t]])
        assert np.array_equal(i1[0], idx[t]) and n1[0] == nm[t]
    perm = np.random.default_rng(3).permutation(11)
    ip, n_p = chain.search(cur, [tg[t] for t in perm])
    assert np.array_equal(ip, idx[perm]) and np.array_equal(n_p, nm[perm])
    again = chain.search(cur, tg)                                          # run twice: the same bits
    assert again[0].tobytes() == idx.tobytes() and again[1].tobytes() == nm.tobytes()


def test_refusals_leave_the_handle_usable(oracle, capi):
    h = capi.BowTargets()
    sc = bts.scene(0, 3, dup=0.3)
    cur, tg = sc["cur"], sc["targets"]
    want_ids, want_nm = bts.oracle_rows(oracle, cur, tg)

    def refused(code, fn):
        with pytest.raises(capi.DvmError) as e:
            fn()
        assert e.value.code == code
        if h_reserved:
            idx, nm = h.search(cur, tg)                                    # ... a valid call on the same handle succeeds
            assert np.array_equal(bts.ids_of(tg, idx), want_ids) and np.array_equal(nm, want_nm)
    h_reserved = False
    refused(-3, lambda: h.search(cur, tg))                                 # nothing reserved
    h.reserve(400, 3, 3 * 400)
    h_reserved = True
    big = bts.scene(0, 11)
    refused(-3, lambda: h.search(cur, big["targets"][:4]))                 # more targets than reserved
    refused(-3, lambda: h.search(cur, [bts.scene(1, 1, n_pts=1300)["targets"][0]]))   # their keypoints beyond the reservation
    refused(-3, lambda: h.search(bts.scene(1, 1, n_pts=500)["cur"], tg))   # the current keyframe beyond the reservation

    def fv_changed(kf, **kw):
        return dict(kf, fv=dict(kf["fv"], **kw))
    nodes, off, feat = (tg[1]["fv"][k] for k in ("fv_nodes", "fv_off", "fv_feat"))
    n = 8193
    huge = bts.make_kf(np.zeros((n, 32), np.uint8), np.zeros(n), np.zeros(n), np.zeros(n, np.uint8), np.zeros(n))
    refused(-1, lambda: h.search(cur, [tg[0], huge]))                      # n > 8192
    refused(-1, lambda: h.search(huge, tg))
    refused(-1, lambda: h.search(cur, [dict(tg[0], desc=None)]))           # a missing array
    refused(-1, lambda: h.search(dict(cur, mp=None), tg))
    refused(-1, lambda: h.search(cur, [fv_changed(tg[0], fv_feat=None)]))
    refused(-1, lambda: h.search(cur, [tg[0], fv_changed(tg[1], fv_nodes=nodes[::-1].copy())]))      # descending nodes
    same = nodes.copy(); same[4] = same[3]
    refused(-1, lambda: h.search(cur, [fv_changed(tg[1], fv_nodes=same)]))                           # ... not strictly ascending
    signed = nodes.copy(); signed[0] = -1
    refused(-1, lambda: h.search(cur, [fv_changed(tg[1], fv_nodes=signed)]))                         # ... ascending as signed only
    o = off.copy(); o[0] = 1
    refused(-1, lambda: h.search(cur, [fv_changed(tg[1], fv_off=o)]))                                # fv_off not from 0
    o = off.copy(); o[5] = o[4] - 1
    refused(-1, lambda: h.search(cur, [fv_changed(tg[1], fv_off=o)]))                                # ... decreasing
    f = feat.copy(); f[7] = len(tg[1]["desc"])
    refused(-1, lambda: h.search(cur, [fv_changed(tg[1], fv_feat=f)]))                               # a feature outside [0, n)
    f = feat.copy(); f[7] = -1
    refused(-1, lambda: h.search(cur, [fv_changed(tg[1], fv_feat=f)]))
    f = feat.copy(); f[-1] = f[0]
    refused(-1, lambda: h.search(cur, [fv_changed(tg[1], fv_feat=f)]))                               # a feature listed twice
    f = cur["fv"]["fv_feat"].copy(); f[3] = f[90]
    refused(-1, lambda: h.search(fv_changed(cur, fv_feat=f), tg))                                    # ... in the current keyframe
    h.close()


def test_host_entry(capi):
    """dvmh_search_by_bow_targets against dvmh_search_by_bow_kf_kf target by target, idx2 included."""
    sc = bts.scene(0, 11, dup=0.3)
    cur, tg = sc["cur"], sc["targets"] + [bts.empty_kf()]
    KF1 = capi.keyframe_view(cur)
    views = [capi.keyframe_view(k) for k in tg]
    for nnratio, check_ori in ((0.9, True), (0.6, False)):
        total, m12, idx2, nm = capi.search_by_bow_targets(KF1, views, nnratio, check_ori)
        for t, v in enumerate(views):
            n_t, row, _ = capi.search_by_bow_kf_kf(KF1, v, nnratio, check_ori)
            assert n_t == nm[t] and np.array_equal(row, m12[t])
        assert np.array_equal(bts.ids_of(tg, idx2), m12) and total == nm.sum() > 400
        assert np.all((idx2 >= 0) == (m12 >= 0))
    total2, m12b, none, nmb = capi.search_by_bow_targets(KF1, views[:3], 0.6, False, want_idx2=False)   # fewer targets on the grown handle, no idx2
    assert none is None and np.array_equal(m12b, m12[:3]) and np.array_equal(nmb, nm[:3]) and total2 == nm[:3].sum()


def test_full_size(oracle, capi):
    """The call's real size: 33 targets of about 1 150 keypoints (three candidates with ten covisibles each)."""
    sc = bts.scene(2, 33, n_pts=1000, n_clutter=250, n_nodes=300, dup=0.1, heavy_frac=0.1)
    assert 1100 <= len(sc["cur"]["desc"]) <= 1200
    h = capi.BowTargets()
    h.reserve(1300, 33, 33 * 1300)
    _, nm = _check(oracle, h, sc["cur"], sc["targets"])
    h.close()
    assert nm.min() > 150
