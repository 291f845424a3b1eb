"""Vocabulary trees shaped like the ones DBoW2 builds, and an independent numpy restatement of TemplatedVocabulary::transform.

synth.vocabulary makes full-depth trees of 2..10 random children.  HKmeansStep (TemplatedVocabulary.h:563-690) does not: a cluster of
one descriptor becomes a leaf above level L, a node of few descriptors has fewer than k children, equal descriptors give equal centres,
and loadFromTextFile takes k up to 20.  dbow2_tree builds such trees; walk() is the transform written once more, without the oracle."""
import functools

import numpy as np

# the scenes of tests/test_voc_scene.py and tests/test_gpu_vocab_trees.py: (k, L) -> generator arguments.  The seeds were chosen on the
# CPU so that every condition test_voc_scene.py asserts holds (the counts as measured are in docs/NOTEBOOK.md).
TREES = {
    (10, 4): dict(seed=7, leaf_frac=0.3, tie_frac=0.1),
    (16, 3): dict(seed=7, leaf_frac=0.3, tie_frac=0.1),
    (17, 3): dict(seed=7, leaf_frac=0.3, tie_frac=0.1),
    (20, 3): dict(seed=2, leaf_frac=0.3, tie_frac=0.1),
    (3, 6): dict(seed=7, leaf_frac=0.15, tie_frac=0.1),
}
N_FEATS = 2000
_POP8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.int64)


def dbow2_tree(k, L, seed, leaf_frac=0.3, kmin=1, tie_frac=0.1):
    """A tree as HKmeansStep leaves it, in the dict form of synth.vocabulary.  Node ids breadth-first (every child after its parent),
    kmin..k children per node, a child above level L is a leaf with probability leaf_frac, a fraction tie_frac of the nodes repeat an
    elder sibling's descriptor, word ids in node order over the leaves, a few words of weight 0."""
    rng = np.random.default_rng(seed)
    kids = {}
    level = [0]
    frontier = [0]
    for d in range(L):
        nxt = []
        for node in frontier:
            kk = int(rng.integers(kmin, k + 1))
            kids[node] = list(range(len(level), len(level) + kk))
            level.extend([d + 1] * kk)
            nxt.extend(c for c in kids[node] if d + 1 < L and rng.random() >= leaf_frac)
        frontier = nxt
    n = len(level)
    level = np.array(level)
    child_off = np.zeros(n + 1, np.int32)
    children = []
    for node in range(n):
        children.extend(kids.get(node, []))
        child_off[node + 1] = len(children)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for node in range(n):
        ch = kids.get(node, [])
        for j in range(1, len(ch)):
            if rng.random() < tie_frac:
                desc[ch[j]] = desc[ch[int(rng.integers(0, j))]]
    leaves = np.flatnonzero(np.diff(child_off) == 0)
    word_id = np.full(n, -1, np.int32)
    word_id[leaves] = np.arange(len(leaves), dtype=np.int32)
    weight = np.zeros(n, np.float64)
    weight[leaves] = np.log(rng.uniform(1.5, 400.0, len(leaves)))
    weight[leaves[rng.random(len(leaves)) < 0.02]] = 0.0
    return dict(n_nodes=n, child_off=child_off, children=np.array(children, np.int32), desc=desc, weight=weight, word_id=word_id, L=L,
                level=level)


def features(voc, n=N_FEATS, seed=0, n_random=100):
    """n features: node descriptors with 5 % of their bytes flipped -- the node drawn from a level drawn first, so that the few nodes
    near the root are walked to as often as the many at level L -- the first n_random of them random."""
    rng = np.random.default_rng(seed)
    by_level = [np.flatnonzero(voc["level"] == d) for d in range(1, voc["L"] + 1)]
    by_level = [b for b in by_level if len(b)]
    node = np.array([rng.choice(by_level[int(rng.integers(0, len(by_level)))]) for _ in range(n)])
    feats = voc["desc"][node].copy()
    feats[rng.random(feats.shape) < 0.05] ^= 0x81
    feats[:n_random] = rng.integers(0, 256, (n_random, 32), dtype=np.uint8)
    return feats


@functools.lru_cache(maxsize=None)
def scene(k, L):
    """(voc, feats, descend(voc, feats)) of one of TREES, made once and shared: read, never written."""
    voc = dbow2_tree(k, L, **TREES[(k, L)])
    feats = features(voc, seed=1000 * k + L)
    return voc, feats, descend(voc, feats)


def descend(voc, feats):
    """The walk itself, which no levelsup changes: path[f, l - 1] = the node feature f reaches at level l (-1 below its leaf), and per
    feature depth (the leaf's level), tie (some level had two children at the minimum) and late (a winner at child position >= 16).
    A strict '<' scan over the children in list order: the first child wins a tie."""
    feats = np.ascontiguousarray(feats, np.uint8).reshape(-1, 32)
    n, off, ch = len(feats), voc["child_off"], voc["children"]
    path = np.full((n, voc["L"]), -1, np.int32)
    depth = np.zeros(n, np.int32); tie = np.zeros(n, bool); late = np.zeros(n, bool)
    for f in range(n):
        cur, lvl = 0, 0
        while True:
            c = ch[off[cur]:off[cur + 1]]
            d = _POP8[voc["desc"][c] ^ feats[f]].sum(axis=1)
            best, pos = int(d[0]), 0
            for j in range(1, len(c)):
                if int(d[j]) < best:
                    best, pos = int(d[j]), j
            tie[f] |= int((d == best).sum()) > 1
            late[f] |= pos >= 16
            cur = int(c[pos])
            path[f, lvl] = cur
            lvl += 1
            if off[cur + 1] == off[cur]:
                break
        depth[f] = lvl
    return dict(path=path, depth=depth, tie=tie, late=late)


def walk(voc, feats, levelsup, down=None):
    """TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup) with TF_IDF / L1_NORM, in numpy (down = descend(voc,
    feats) where the caller has it): the leaf gives word and weight; the node at level L - levelsup is the feature's node id -- 0 when
    that level is <= 0, -1 when the leaf lies above it.  Features of weight 0 enter neither vector.  Returns the outputs of
    oracle.vocab_transform (the FeatureVector in std::map<unsigned> order) plus fv = {unsigned node: [features]} and descend's depth,
    tie and late."""
    down = down or descend(voc, feats)
    path, depth, tie, late = down["path"], down["depth"], down["tie"], down["late"]
    n = len(path)
    leaf = path[np.arange(n), depth - 1]
    word, weight = voc["word_id"][leaf].astype(np.int32), voc["weight"][leaf].astype(np.float64)
    nid_level = voc["L"] - levelsup
    node = np.zeros(n, np.int32) if nid_level <= 0 else path[:, nid_level - 1].copy()
    bow, fv = {}, {}
    for f in range(n):
        if weight[f] > 0:
            bow[int(word[f])] = bow.get(int(word[f]), 0.0) + float(weight[f])
            fv.setdefault(int(node[f]) & 0xFFFFFFFF, []).append(f)
    ids = sorted(bow)
    norm = 0.0
    for i in ids:
        norm += abs(bow[i])
    vals = [bow[i] / norm if norm > 0.0 else bow[i] for i in ids]
    nodes = sorted(fv)
    return dict(word=word, node=node, weight=weight, bow_ids=np.array(ids, np.int32), bow_vals=np.array(vals, np.float64),
                fv_nodes=np.array(nodes, np.uint32).astype(np.int32), fv_off=np.cumsum([0] + [len(fv[x]) for x in nodes]).astype(np.int32),
                fv_feat=np.array([f for x in nodes for f in fv[x]], np.int32), fv=fv, depth=depth, tie=tie, late=late)


def write_dbow2_text(voc, path, k):
    """The vocabulary in DBoW2's text form (saveToTextFile, TemplatedVocabulary.h:1290-1315): "k L scoring weighting", then one line per
    node in id order: parent, isLeaf, 32 descriptor bytes, weight.  synth.vocabulary and dbow2_tree number their nodes breadth-first,
    children after parents, as a file read by loadFromTextFile does; the leaf flag stands wherever the node has no children."""
    parent = np.zeros(voc["n_nodes"], np.int64)
    for n in range(voc["n_nodes"]):
        parent[voc["children"][voc["child_off"][n]:voc["child_off"][n + 1]]] = n
    with open(path, "w") as f:
        f.write(f"{k} {voc['L']}  0 0\n")
        for n in range(1, voc["n_nodes"]):
            leaf = int(voc["word_id"][n] >= 0)
            f.write(f"{parent[n]} {leaf} " + " ".join(str(int(b)) for b in voc["desc"][n]) + f" {float(voc['weight'][n])!r}\n")
        f.write("\n")                                  # ORBvoc.txt ends in a newline; the loader must not turn it into a node


def fv_from_nodes(node):
    """The FeatureVector (CSR dict) of per-feature node ids, nodes in std::map<unsigned> order, a node's features ascending."""
    u = np.asarray(node, np.int64) & 0xFFFFFFFF
    nodes, counts = np.unique(u, return_counts=True)
    return dict(fv_nodes=nodes.astype(np.uint32).astype(np.int32), fv_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                fv_feat=np.argsort(u, kind="stable").astype(np.int32))


def node_of_feature(fv, n):
    """Per-feature node id (int64, unsigned value; -2 = in no node) of a CSR FeatureVector over n features."""
    out = np.full(n, -2, np.int64)
    for a, x in enumerate(fv["fv_nodes"]):
        out[fv["fv_feat"][fv["fv_off"][a]:fv["fv_off"][a + 1]]] = int(x) & 0xFFFFFFFF
    return out


# ---- keyframe pairs whose FeatureVectors end in node -1, and what the three FeatureVector walks of ORBmatcher must return on them ----------
PAIR_VARIANTS = ("5_7", "3_2", "tree")


@functools.lru_cache(maxsize=None)
def neg_node_pair(variant, seed=5):
    """matcher_scene.make_kf_pair_scene without duplicates (conflict-free), its vocabulary nodes replaced.  "5_7" / "3_2": the features of
    half of the nodes go to node -1 in both keyframes, the rest to node 5 (3) in the first keyframe and 7 (2) in the second -- node -1 is
    the one node they share, and it is the last of either list.  "tree": each keyframe's descriptors through walk() on the (10, 4) tree
    with levelsup 1.  Returns (kf1, kf2); read, never written."""
    from matcher_scene import make_kf_pair_scene
    from oracle import pyoracle as po
    a, b = make_kf_pair_scene(po, seed=seed, dup_frac=0.0)["kf"]
    out = []
    for v, kf in enumerate((a, b)):
        if variant == "tree":
            voc = scene(10, 4)[0]
            w = walk(voc, kf["desc"], 1)
            fv = {k: w[k] for k in ("fv_nodes", "fv_off", "fv_feat")}
        else:
            low = (int(variant[0]), int(variant[2]))[v]
            node = node_of_feature(kf["fv"], len(kf["kps"]))
            fv = fv_from_nodes(np.where((node - 3) // 7 >= 60, -1, low))
        out.append(dict(kf, fv=fv))
    return tuple(out)


def _ham(a, b):
    return int(_POP8[a ^ b].sum())


def _by_node(fv):
    return {int(x) & 0xFFFFFFFF: [int(f) for f in fv["fv_feat"][fv["fv_off"][a]:fv["fv_off"][a + 1]]] for a, x in enumerate(fv["fv_nodes"])}


def brute_bow(kf1, kf2, nnratio, to_frame):
    """SearchByBoW by definition, nodes keyed as unsigned: every feature of kf1 that holds a good map point takes, among the features of
    its node in kf2, the one of smallest distance if that is within TH_LOW and passes the ratio test against the second smallest.
    to_frame: SearchByBoW(KF, F) -- every F feature is a candidate, distance <= 50; else SearchByBoW(KF1, KF2) -- candidates hold a good
    map point, distance < 50.  Without the claims of the sequential loop and without the histogram: valid where no kf2 feature is taken
    twice (asserted).  Returns {kf1 feature: (kf2 feature, unsigned node)}."""
    n1, n2 = _by_node(kf1["fv"]), _by_node(kf2["fv"])
    out = {}
    for node in sorted(set(n1) & set(n2)):
        c2 = [j for j in n2[node] if to_frame or (kf2["mp"][j] >= 0 and not kf2["bad"][j])]
        for i in n1[node]:
            if kf1["mp"][i] < 0 or kf1["bad"][i] or not c2:
                continue
            d = sorted((_ham(kf1["desc"][i], kf2["desc"][j]), k) for k, j in enumerate(c2))
            b1 = d[0][0]; b2 = d[1][0] if len(d) > 1 else 256
            if (b1 <= 50 if to_frame else b1 < 50) and np.float32(b1) < np.float32(nnratio) * np.float32(b2):
                out[i] = (c2[d[0][1]], node)
    assert len({j for j, _ in out.values()}) == len(out), "the scene has conflicts"
    return out


def brute_triangulation(kf1, kf2, ep):
    """SearchForTriangulation (coarse, no orientation check) by definition, nodes keyed as unsigned: a kf1 feature without a map point
    takes, among the features without one of its node in kf2 that lie outside the epipole's disc, the one of smallest distance <= 50,
    the last of them in the node's order.  Returns {kf1 feature: (kf2 feature, unsigned node)}."""
    n1, n2 = _by_node(kf1["fv"]), _by_node(kf2["fv"])
    f32 = np.float32
    out = {}
    for node in sorted(set(n1) & set(n2)):
        for i in n1[node]:
            if kf1["mp"][i] >= 0:
                continue
            best = (51, -1)
            for j in n2[node]:
                if kf2["mp"][j] >= 0:
                    continue
                d = _ham(kf1["desc"][i], kf2["desc"][j])
                ex, ey = f32(ep[0]) - kf2["kps"]["x"][j], f32(ep[1]) - kf2["kps"]["y"][j]
                if f32(f32(ex * ex) + f32(ey * ey)) < f32(100) * kf2["scale_factors"][kf2["kps"]["octave"][j]]:
                    continue
                if d <= 50 and d <= best[0]:
                    best = (d, j)
            if best[1] >= 0:
                out[i] = (best[1], node)
    return out


def fold_new_points_scene(sc, from_index=35):
    """A new_points_scene scene (new_points_scene.prefix: fresh map-point table) whose nodes 7 i + 3 with i >= from_index are node -1 in
    the current keyframe and in every neighbour: each FeatureVector ends in node -1."""
    def fold(kf):
        node = node_of_feature(kf["fv"], len(kf["kps"]))
        return dict(kf, fv=fv_from_nodes(np.where((node - 3) // 7 >= from_index, -1, node)))
    return dict(cur=fold(sc["cur"]), neighbours=[fold(kf) for kf in sc["neighbours"]], median_depth=sc["median_depth"])
