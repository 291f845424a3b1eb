"""The bag-of-words path on vocabulary trees shaped like DBoW2's (tests/voc_scene.py: leaves above level L, 1..20 children, equal
siblings) and on FeatureVectors that end in node -1.  k_vocab_transform through both forms of dvm_vocab_transform, the host transform and
the text loader against the numpy walk and the oracle; the three FeatureVector walks of the host matcher against brute-force definitions
keyed by unsigned node; dvm_create_new_map_points[_cam] with candidates inside node -1; dvm_vocab_create's refusal of lists that are no
tree.  Every comparison is exact: integers equal, doubles bit for bit."""
import numpy as np
import pytest

import new_points_scene as nps
import voc_scene as vs

pytestmark = pytest.mark.gpu

NEG = 0xFFFFFFFF
FV_KEYS = ("bow_ids", "bow_vals", "fv_nodes", "fv_off", "fv_feat")


def _levelsups(L):
    return (0, 1, 2, L, L + 2)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("k,L", list(vs.TREES))
def test_transform_equals_walk_and_oracle(capi, oracle, k, L):
    voc, feats, down = vs.scene(k, L)
    v = capi.Vocabulary(voc)
    for levelsup in _levelsups(L):
        w = vs.walk(voc, feats, levelsup, down)
        r = oracle.vocab_transform(voc, feats, levelsup)
        for n in (1, 15, 16, 17, vs.N_FEATS):              # a row of a wave, a workgroup of 16 rows less one, full, and one more
            for on_device in (False, True):
                word, node, weight = v.transform(feats[:n], levelsup, on_device=on_device)
                for got, key in ((word, "word"), (node, "node")):
                    assert np.array_equal(got, w[key][:n]) and np.array_equal(got, r[key][:n]), (levelsup, n, on_device, key)
                assert np.array_equal(_bits(weight), _bits(w["weight"][:n])) and np.array_equal(_bits(weight), _bits(r["weight"][:n]))
        h = capi.vocab_transform_host(voc, feats, levelsup)
        for key in FV_KEYS:
            assert np.array_equal(h[key], r[key]) and np.array_equal(h[key], w[key]), (levelsup, key)
        assert np.array_equal(_bits(h["bow_vals"]), _bits(r["bow_vals"]))
        if levelsup == 1:
            assert h["fv_nodes"][-1] == -1 and (node == -1).sum() >= 100
    v.close()


@pytest.mark.parametrize("k,L", [(20, 3), (3, 6)])
def test_text_vocabulary_with_early_leaves(capi, oracle, tmp_path, k, L):
    """loadFromTextFile on a file with leaf flags above level L (and k = 20, the most it takes): the transform of the tree it was
    written from."""
    voc, feats, down = vs.scene(k, L)
    path = tmp_path / "voc.txt"
    vs.write_dbow2_text(voc, path, k)
    hv = capi.HostVocabulary(str(path))
    assert (hv.k, hv.L, hv.nodes, hv.words) == (k, L, voc["n_nodes"], int((voc["word_id"] >= 0).sum()))
    for levelsup in _levelsups(L):
        h = hv.transform(feats, levelsup)
        r = oracle.vocab_transform(voc, feats, levelsup)
        w = vs.walk(voc, feats, levelsup, down)
        for key in FV_KEYS:
            assert np.array_equal(h[key], r[key]) and np.array_equal(h[key], w[key]), (levelsup, key)
        assert np.array_equal(_bits(h["bow_vals"]), _bits(r["bow_vals"]))
    hv.close()
    text = path.read_text().splitlines()
    bad = tmp_path / "bad.txt"
    bad.write_text("\n".join([f"21 {L}  0 0"] + text[1:]) + "\n")
    with pytest.raises(RuntimeError):
        capi.HostVocabulary(str(bad))


def test_vocab_create_refuses_what_is_no_tree(capi):
    """A child list with a back edge, a self edge, or a node under two parents is refused when the vocabulary is made -- the walk of
    k_vocab_transform would not leave the first two.  Nothing is ever transformed on such a list."""
    voc = vs.scene(3, 6)[0]
    off, ch = voc["child_off"], voc["children"]
    parent = np.zeros(voc["n_nodes"], np.int64)
    parent[ch] = np.repeat(np.arange(voc["n_nodes"]), np.diff(off))
    inner = [i for i in range(1, voc["n_nodes"]) if off[i + 1] > off[i] and parent[i] > 0]
    i = inner[-1]                                          # an inner node at depth >= 2
    other = max(j for j in range(i + 1, voc["n_nodes"]) if parent[j] != i)      # a node after i that another parent lists

    def refused(what, value):
        c = ch.copy(); c[off[i]] = value
        with pytest.raises(capi.DvmError) as e:
            capi.Vocabulary(dict(voc, children=c))
        assert e.value.code == -1 and "vocabulary" in str(e.value), what
    refused("a back edge to the grandparent", parent[parent[i]])
    refused("a back edge to the parent", parent[i])
    refused("a self edge", i)
    refused("a node under two parents (and another under none)", other)
    v = capi.Vocabulary(voc)                               # the tree itself is taken
    v.close()


def _views(capi, a, b):
    da, db = dict(a, mp=a["mp"].copy()), dict(b, mp=b["mp"].copy())
    return capi.keyframe_view(da), capi.keyframe_view(db)


@pytest.mark.parametrize("variant", vs.PAIR_VARIANTS)
def test_host_matcher_walks_nodes_unsigned(capi, oracle, variant):
    """SearchByBoW x2 and SearchForTriangulation of the host library on keyframes whose FeatureVectors end in node -1."""
    a, b = vs.neg_node_pair(variant)
    if variant == "tree":                                  # the lists are what this library's own transform gives
        voc = vs.scene(10, 4)[0]
        for kf in (a, b):
            h = capi.vocab_transform_host(voc, kf["desc"], 1)
            assert all(np.array_equal(h[key], kf["fv"][key]) for key in ("fv_nodes", "fv_off", "fv_feat")) and h["fv_nodes"][-1] == -1
    va, vb = _views(capi, a, b)
    ref = vs.brute_bow(a, b, 0.8, to_frame=False)
    assert sum(node == NEG for _, node in ref.values()) >= 10
    for ori in (False, True):
        n_g, m_g, _ = capi.search_by_bow_kf_kf(va, vb, 0.8, ori)
        n_o, m_o = oracle.search_by_bow_kf_kf(a["kps"], a["desc"], a["mp"], a["bad"], a["fv"], b["kps"], b["desc"], b["mp"], b["bad"], b["fv"], 0.8, ori)
        assert n_g == n_o and np.array_equal(m_g, m_o)
        if not ori:
            assert n_g == len(ref) and {int(i): int(m_g[i]) for i in np.flatnonzero(m_g >= 0)} == {i: int(b["mp"][j]) for i, (j, _) in ref.items()}
    ref = vs.brute_bow(a, b, 0.7, to_frame=True)
    assert sum(node == NEG for _, node in ref.values()) >= 10
    F = capi.frame_view(b["kps"], b["desc"], b["bounds"], b["scale_factors"])
    for ori in (False, True):
        n_g, m_g, _ = capi.search_by_bow_kf_frame(va, F, b["fv"], 0.7, ori)
        n_o, m_o = oracle.search_by_bow_kf_frame(a["kps"], a["desc"], a["mp"], a["bad"], a["fv"], b["kps"], b["desc"], b["fv"], 0.7, ori)
        assert n_g == n_o and np.array_equal(m_g, m_o)
        if not ori:
            assert n_g == len(ref) and {int(j): int(m_g[j]) for j in np.flatnonzero(m_g >= 0)} == {j: int(a["mp"][i]) for i, (j, _) in ref.items()}
    geo = oracle.triangulation_geometry(a["Tcw"], b["Tcw"], a["K"], b["K"])
    ref = vs.brute_triangulation(a, b, geo[2])
    assert sum(node == NEG for _, node in ref.values()) >= 10
    for coarse, ori in ((True, False), (False, True)):
        n_g, p_g = capi.search_for_triangulation(va, vb, coarse, ori)
        n_o, p_o = oracle.search_for_triangulation(a["kps"], a["desc"], a["mp"], a["fv"], b["kps"], b["desc"], b["mp"], b["fv"], geo[3], geo[2],
                                                   b["scale_factors"], b["level_sigma2"], coarse, ori)
        assert n_g == n_o and np.array_equal(p_g, p_o)
        if coarse:
            assert n_g == len(ref) and [tuple(p) for p in p_g.tolist()] == [(i, ref[i][0]) for i in sorted(ref)]
        else:
            node1 = vs.node_of_feature(a["fv"], len(a["kps"]))
            assert (node1[p_g[:, 0]] == NEG).sum() >= 10


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.NewPoints()
    h.reserve(2048, 5, 5 * 1024)
    yield h
    h.close()


def _pairs_in_neg(sc, got):
    return int((vs.node_of_feature(sc["cur"]["fv"], len(sc["cur"]["kps"]))[got["pairs"][:, 0]] == NEG).sum())


@pytest.mark.parametrize("variant", [dict(), dict(check_ori=True)])
def test_new_points_take_lists_that_end_in_node_minus_one(capi, chain, variant):
    """dvm_create_new_map_points accepts keyframes whose FeatureVectors end in node -1 and finds the candidates inside it."""
    sc = vs.fold_new_points_scene(nps.prefix(nps.scene(0), 5))
    assert sc["cur"]["fv"]["fv_nodes"][-1] == -1 and all(kf["fv"]["fv_nodes"][-1] == -1 for kf in sc["neighbours"])
    want = nps.oracle_chain(vs.fold_new_points_scene(nps.prefix(nps.scene(0), 5)), **variant)
    got = chain.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"], **variant)
    nps.assert_same(got, want)
    assert _pairs_in_neg(sc, got) >= 10 and (got["status"] == 0).sum() >= 30
    nps.assert_same(capi.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"], **variant), want)


def test_new_points_cam_take_lists_that_end_in_node_minus_one(capi, chain):
    """... and so does the KannalaBrandt8 form, whose kernels share the node lookup: against the loop of the two _cam calls."""
    import kb8_tri_scene as kt
    import test_gpu_kb8_new_points as kb
    sc = vs.fold_new_points_scene(nps.prefix(kt.chain_scene(0), 5))
    got = kb._run(capi, chain, sc, check_ori=True)
    want = kb._separate_calls(capi, vs.fold_new_points_scene(nps.prefix(kt.chain_scene(0), 5)), check_ori=True)
    nps.assert_same(got, want)
    assert _pairs_in_neg(sc, got) >= 10 and (got["status"] == 0).sum() >= 30


def test_new_points_refuse_node_minus_one_first(capi, chain):
    """A list that ascends as signed only (-1 first) is refused, as by the BoW chain; the handle serves the next call."""
    sc = vs.fold_new_points_scene(nps.prefix(nps.scene(0), 5))
    want = chain.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"])

    def signed(kf):
        fv = kf["fv"]
        sizes = np.diff(fv["fv_off"])
        feat = np.concatenate([fv["fv_feat"][fv["fv_off"][-2]:], fv["fv_feat"][:fv["fv_off"][-2]]])
        return dict(kf, fv=dict(fv_nodes=np.roll(fv["fv_nodes"], 1), fv_off=np.concatenate([[0], np.cumsum(np.roll(sizes, 1))]).astype(np.int32),
                                fv_feat=feat.astype(np.int32)))
    assert signed(sc["cur"])["fv"]["fv_nodes"][0] == -1 and np.all(np.diff(signed(sc["cur"])["fv"]["fv_nodes"]) > 0)
    for cur, nbs in ((signed(sc["cur"]), sc["neighbours"]), (sc["cur"], sc["neighbours"][:2] + [signed(sc["neighbours"][2])] + sc["neighbours"][3:])):
        with pytest.raises(capi.DvmError) as e:
            chain.create_new_map_points(cur, nbs, sc["median_depth"])
        assert e.value.code == -1 and "ascending" in str(e.value)
        nps.assert_same(chain.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"]), want)
