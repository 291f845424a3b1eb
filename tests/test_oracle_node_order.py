"""FeatureVector nodes ascend as unsigned; -1 is last.  The oracle's three FeatureVector walks (SearchByBoW keyframe to frame and
keyframe to keyframe, SearchForTriangulation) against brute-force numpy definitions keyed by unsigned node (tests/voc_scene.py), on
keyframe pairs whose lists end in node -1: a walk that compares node ids as signed jumps past the shared last node and finds nothing
there."""
import numpy as np
import pytest

import voc_scene as vs
from oracle import pyoracle as po

NEG = 0xFFFFFFFF


def _ends_in_neg(kf):
    n = kf["fv"]["fv_nodes"]
    return n[-1] == -1 and np.all(np.diff(n.astype(np.uint32).astype(np.int64)) > 0)


@pytest.mark.parametrize("variant", vs.PAIR_VARIANTS)
def test_search_by_bow_walks_unsigned(variant):
    a, b = vs.neg_node_pair(variant)
    assert _ends_in_neg(a) and _ends_in_neg(b)
    ref = vs.brute_bow(a, b, 0.8, to_frame=False)
    n, m12 = po.search_by_bow_kf_kf(a["kps"], a["desc"], a["mp"], a["bad"], a["fv"], b["kps"], b["desc"], b["mp"], b["bad"], b["fv"], 0.8, False)
    assert sum(node == NEG for _, node in ref.values()) >= 10, "matches inside node -1"
    assert n == len(ref) and {int(i): int(m12[i]) for i in np.flatnonzero(m12 >= 0)} == {i: int(b["mp"][j]) for i, (j, _) in ref.items()}
    ref = vs.brute_bow(a, b, 0.7, to_frame=True)
    n, mf = po.search_by_bow_kf_frame(a["kps"], a["desc"], a["mp"], a["bad"], a["fv"], b["kps"], b["desc"], b["fv"], 0.7, False)
    assert sum(node == NEG for _, node in ref.values()) >= 10
    assert n == len(ref) and {int(j): int(mf[j]) for j in np.flatnonzero(mf >= 0)} == {j: int(a["mp"][i]) for i, (j, _) in ref.items()}


@pytest.mark.parametrize("variant", vs.PAIR_VARIANTS)
def test_search_for_triangulation_walks_unsigned(variant):
    a, b = vs.neg_node_pair(variant)
    _, _, ep, F12 = po.triangulation_geometry(a["Tcw"], b["Tcw"], a["K"], b["K"])
    ref = vs.brute_triangulation(a, b, ep)
    n, pairs = po.search_for_triangulation(a["kps"], a["desc"], a["mp"], a["fv"], b["kps"], b["desc"], b["mp"], b["fv"], F12, ep,
                                           b["scale_factors"], b["level_sigma2"], coarse=True, check_ori=False)
    assert sum(node == NEG for _, node in ref.values()) >= 10, "pairs inside node -1"
    assert n == len(ref) and [tuple(p) for p in pairs.tolist()] == [(i, ref[i][0]) for i in sorted(ref)]
