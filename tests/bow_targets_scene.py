"""Scenes for dvm_search_by_bow_targets (one current keyframe against T target keyframes: the SearchByBoW calls of
LoopClosing::DetectCommonRegionsFromBoW), in the manner of matcher_scene.make_kf_pair_scene: all keyframes observe the same 3-D points
(+ clutter), a point's keypoints share a vocabulary node in every view (with a few defects) and differ by a few descriptor bits, about
half the keypoints carry a map point (some of them bad), a fraction of the points are near-duplicates that compete for one candidate, and
one heavy node holds more than 64 usable features.  walk() restates ORBmatcher.cc:709-834 in Python with the bookkeeping the tests ask
about; tests/test_oracle_bow_targets.py pins it to the oracle and pins what the scenes contain."""
import functools

import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
BOUNDS = np.array([0.0, 640.0, 0.0, 480.0], np.float32)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
TH_LOW = 50


def flip(rng, d, nbits):
    """d with exactly nbits[r] (or nbits) distinct bits of every row flipped."""
    d = np.array(d, np.uint8, copy=True).reshape(-1, 32)
    nb = np.broadcast_to(np.asarray(nbits), (len(d),))
    for r in range(len(d)):
        for b in rng.choice(256, int(nb[r]), replace=False):
            d[r, b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def make_kf(desc, node, mp, bad, angle, rng=None):
    """A keyframe dict (what capi.keyframe_view / capi.BowTargets take) from per-keypoint arrays; the FeatureVector lists the nodes
    ascending as unsigned and a node's features ascending, as DBoW2 builds it (a negative id sorts last); drop_features() takes keypoints out of it."""
    n = len(desc)
    kps = np.zeros(n, KP_DTYPE)
    kps["angle"] = np.asarray(angle, np.float32)
    if rng is not None:
        kps["x"] = rng.uniform(5, 635, n); kps["y"] = rng.uniform(5, 475, n); kps["octave"] = rng.integers(0, 8, n)
    node = np.asarray(node, np.int64).astype(np.int32)
    order = np.argsort(node.view(np.uint32), kind="stable")
    nodes, counts = np.unique(node.view(np.uint32), return_counts=True)
    fv = dict(fv_nodes=nodes.view(np.int32).copy(), fv_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), fv_feat=order.astype(np.int32))
    return dict(kps=kps, desc=np.ascontiguousarray(desc, np.uint8).reshape(n, 32), mp=np.ascontiguousarray(mp, np.int32),
                bad=np.ascontiguousarray(bad, np.uint8), fv=fv, bounds=BOUNDS, node=node)


@functools.lru_cache(maxsize=None)
def scene(seed=0, T=3, n_pts=330, n_clutter=70, n_nodes=40, dup=0.0, mapped_frac=0.5, bad_frac=0.06, flip_bits=10, heavy_frac=0.6):
    """dict(cur, targets[T]).  Cached: the callers do not modify it (the knobs below return changed copies)."""
    rng = np.random.default_rng(1000 * seed + T)
    base = rng.integers(0, 256, (n_pts, 32), dtype=np.uint8)
    node_of_pt = rng.integers(1, n_nodes, n_pts) * 7 + 3               # sparse ids
    node_of_pt[rng.random(n_pts) < heavy_frac] = 3                      # the heavy node
    ndup = int(dup * n_pts)                                            # near-identical descriptors in one node: they compete
    src = rng.choice(n_pts, ndup, replace=False); dst = rng.choice(np.setdiff1d(np.arange(n_pts), src), ndup, replace=False)
    base[dst] = flip(rng, base[src], 3)
    node_of_pt[dst] = node_of_pt[src]
    mapped = rng.random(n_pts) < mapped_frac / 0.85                    # (clutter is never mapped: about half of all keypoints)
    pt_angle = rng.uniform(0, 360, n_pts)
    kfs = []
    for v in range(T + 1):
        idx = np.nonzero(rng.random(n_pts) < 0.9)[0]
        idx = idx[rng.permutation(len(idx))]
        m = len(idx)
        desc = np.concatenate([flip(rng, base[idx], flip_bits), rng.integers(0, 256, (n_clutter, 32), dtype=np.uint8)])
        clutter_node = np.where(rng.random(n_clutter) < heavy_frac, 3, rng.integers(1, n_nodes, n_clutter) * 7 + 3)
        node = np.concatenate([np.where(rng.random(m) < 0.92, node_of_pt[idx], rng.integers(1, n_nodes, m) * 7 + 3), clutter_node])
        # most matches share one rotation against the current keyframe, a minority is rotated elsewhere (the histogram takes them back)
        rot = np.where(rng.random(m) < 0.8, 40.0 * (v % 4), rng.uniform(0, 360, m)) if v else np.zeros(m)
        angle = np.concatenate([np.mod(pt_angle[idx] - rot + rng.normal(0, 3, m) + 720.0, 360.0), rng.uniform(0, 360, n_clutter)])
        mp = np.full(m + n_clutter, -1, np.int32)
        mp[:m] = np.where(mapped[idx], 1000 + idx, -1)                 # unique inside a keyframe
        bad = ((mp >= 0) & (rng.random(m + n_clutter) < bad_frac)).astype(np.uint8)
        kfs.append(make_kf(desc, node, mp, bad, angle, rng))
    return dict(cur=kfs[0], targets=kfs[1:])


def edge_scene(k, seed=0, n_cur=24, extra=9):
    """Three nodes; the target's node 10 holds exactly k usable features (+ `extra` unusable ones scattered between them), and the
    current keyframe's n_cur queries of that node match features spread over the whole scan, the last position included."""
    rng = np.random.default_rng(77 * k + seed)
    n_cur = min(n_cur, k)
    tdesc = rng.integers(0, 256, (k + extra, 32), dtype=np.uint8)
    usable = np.ones(k + extra, bool)
    usable[rng.choice(k + extra - 1, extra, replace=False)] = False    # (the last position stays usable)
    upos = np.nonzero(usable)[0]
    hit = np.unique(np.concatenate([rng.choice(upos, n_cur - 1, replace=False), upos[-1:]]))
    tmp = np.where(usable, 500 + np.arange(k + extra), -1)
    tbad = np.zeros(k + extra, np.uint8)
    unus = np.nonzero(~usable)[0]
    tmp[unus[::2]] = 900 + unus[::2]; tbad[unus[::2]] = 1               # half of the unusable ones: a bad point, the others: none
    tangle = rng.uniform(0, 360, k + extra)
    side = 12                                                          # two small side nodes
    sdesc = rng.integers(0, 256, (side, 32), dtype=np.uint8)
    target = make_kf(np.concatenate([tdesc, sdesc]), np.concatenate([np.full(k + extra, 10), np.repeat([4, 20], side // 2)]),
                     np.concatenate([tmp, 700 + np.arange(side)]), np.concatenate([tbad, np.zeros(side, np.uint8)]),
                     np.concatenate([tangle, rng.uniform(0, 360, side)]), rng)
    perm = rng.permutation(len(hit))
    cdesc = np.concatenate([flip(rng, tdesc[hit][perm], 8), flip(rng, sdesc, 6)])
    cur = make_kf(cdesc, np.concatenate([np.full(len(hit), 10), np.repeat([4, 20], side // 2)]), 100 + np.arange(len(cdesc)),
                  np.zeros(len(cdesc), np.uint8), np.concatenate([np.mod(tangle[hit][perm] + 30, 360), rng.uniform(0, 360, side)]), rng)
    return dict(cur=cur, targets=[target], k=k)


def boundary_scene(seed=0):
    """Query 0 of the current keyframe has its best candidate at distance exactly 50 (TH_LOW: unmatched under the strict < of
    ORBmatcher.cc:785, matched under <=), query 1 at exactly 49; every other candidate of their nodes lies 128 bits away, so the ratio
    test passes at 0.9.  Two targets (the second scans the far candidates first) and some ordinary features around them."""
    rng = np.random.default_rng(seed + 5)
    q = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    fill = scene(seed, 2, n_pts=60, n_clutter=10, n_nodes=6, heavy_frac=0.0)
    cur0 = fill["cur"]
    cur = make_kf(np.concatenate([q, cur0["desc"]]), np.concatenate([[900, 901], cur0["node"]]), np.concatenate([[1, 2], cur0["mp"]]),
                  np.concatenate([[0, 0], cur0["bad"]]), np.concatenate([[100.0, 100.0], cur0["kps"]["angle"]]), rng)
    targets = []
    for t in range(2):
        k0 = fill["targets"][t]
        d = np.concatenate([flip(rng, q[0:1], 50), flip(rng, q[1:2], 49)] + [flip(rng, q[i:i + 1], 128) for i in (0, 0, 1, 1)])
        nd = np.array([900, 901, 900, 900, 901, 901])
        order = np.arange(6) if t == 0 else np.array([2, 4, 0, 3, 1, 5])     # the second target scans the far candidates first
        targets.append(make_kf(np.concatenate([d[order], k0["desc"]]), np.concatenate([nd[order], k0["node"]]), np.concatenate([order + 10, k0["mp"]]),
                               np.concatenate([np.zeros(6, np.uint8), k0["bad"]]), np.concatenate([np.full(6, 100.0 - 40.0 * (t + 1)), k0["kps"]["angle"]]), rng))   # (the rotation most of the target's matches have)
    return dict(cur=cur, targets=targets)


# ---- knobs: changed copies of a keyframe dict
def without_map_points(kf):
    return dict(kf, mp=np.full(len(kf["mp"]), -1, np.int32))


def all_bad(kf):
    return dict(kf, bad=(kf["mp"] >= 0).astype(np.uint8))


def empty_kf():
    return make_kf(np.zeros((0, 32), np.uint8), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.float32))


def renoded(kf, node):
    """The same keypoints with other node ids (an int array, or a function of the present ids)."""
    node = node(kf["node"]) if callable(node) else np.broadcast_to(np.asarray(node), kf["node"].shape)
    k = make_kf(kf["desc"], node, kf["mp"], kf["bad"], kf["kps"]["angle"])
    k["kps"] = kf["kps"]
    return k


def drop_features(kf, which):
    """The keypoints `which` leave the FeatureVector (a stopped word: the keypoint stays, no node lists it)."""
    fv = kf["fv"]
    keep = ~np.isin(fv["fv_feat"], which)
    node_of = np.repeat(np.arange(len(fv["fv_nodes"])), np.diff(fv["fv_off"]))[keep]
    counts = np.bincount(node_of, minlength=len(fv["fv_nodes"]))
    live = counts > 0
    return dict(kf, fv=dict(fv_nodes=fv["fv_nodes"][live], fv_off=np.concatenate([[0], np.cumsum(counts[live])]).astype(np.int32),
                            fv_feat=fv["fv_feat"][keep]))


# ---- the reference walk in Python
def usable(kf):
    return (kf["mp"] >= 0) & (kf["bad"] == 0)


def rot_bin(a1, a2):
    """csrc/rot_bin.h in float32 (roundf of a non-negative value: halves away from zero)."""
    rot = np.float32(a1) - np.float32(a2)
    if rot < 0:
        rot = np.float32(rot + np.float32(360.0))
    x = np.float32(rot * (np.float32(1.0) / np.float32(30)))
    b = int(np.floor(x)) + (1 if x - np.floor(x) >= 0.5 else 0)
    return 0 if b == 30 else b


def three_maxima(h):
    m1 = m2 = m3 = 0; i1 = i2 = i3 = -1
    for i, s in enumerate(h):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    if np.float32(m2) < np.float32(0.1) * np.float32(m1):
        i2 = i3 = -1
    elif np.float32(m3) < np.float32(0.1) * np.float32(m1):
        i3 = -1
    return i1, i2, i3


def walk(cur, tgt, nnratio=0.9, check_ori=True, th_low_inclusive=False):
    """SearchByBoW(cur, tgt) as ORBmatcher.cc:709-834 walks it.  Returns (nmatches, idx2[n1], stats) with stats = dict(queries,
    met_claimed: queries whose scan skipped an already-matched candidate, claim_mattered: of those, the ones whose best or second distance
    the skipped candidates would have changed, max_usable: the largest number of usable target features in a common node,
    best: {query keypoint: (best, second)})."""
    f1, f2 = cur["fv"], tgt["fv"]
    u1, u2 = usable(cur), usable(tgt)
    idx2 = np.full(len(cur["desc"]), -1, np.int32)
    matched2 = np.zeros(len(tgt["desc"]), bool)
    rot = [[] for _ in range(30)]
    st = dict(queries=0, met_claimed=0, claim_mattered=0, max_usable=0, best={})
    pos2 = {int(n): b for b, n in enumerate(f2["fv_nodes"].view(np.uint32))}
    nm = 0
    for a, n in enumerate(f1["fv_nodes"].view(np.uint32)):
        b = pos2.get(int(n))
        if b is None:
            continue
        c2 = f2["fv_feat"][f2["fv_off"][b]:f2["fv_off"][b + 1]]
        c2 = c2[u2[c2]]
        st["max_usable"] = max(st["max_usable"], len(c2))
        for i1 in f1["fv_feat"][f1["fv_off"][a]:f1["fv_off"][a + 1]]:
            if not u1[i1]:
                continue
            st["queries"] += 1
            d_all = _POP[cur["desc"][i1][None, :] ^ tgt["desc"][c2]].sum(axis=1) if len(c2) else np.zeros(0, np.int32)
            free = ~matched2[c2]

            def two(d):
                if len(d) == 0:
                    return 256, 256, -1
                o = np.argsort(d, kind="stable")
                return int(d[o[0]]), (int(d[o[1]]) if len(d) > 1 else 256), int(o[0])
            b1, b2, k = two(d_all[free])
            if not free.all():
                st["met_claimed"] += 1
                st["claim_mattered"] += two(d_all)[:2] != (b1, b2)
            st["best"][int(i1)] = (b1, b2)
            ok = (b1 <= TH_LOW if th_low_inclusive else b1 < TH_LOW) and np.float32(b1) < np.float32(nnratio) * np.float32(b2)
            if ok:
                j = int(c2[free][k])
                idx2[i1] = j; matched2[j] = True; nm += 1
                if check_ori:
                    rot[rot_bin(cur["kps"]["angle"][i1], tgt["kps"]["angle"][j])].append(int(i1))
    if check_ori:
        keep = three_maxima([len(r) for r in rot])
        for i, r in enumerate(rot):
            if i not in keep:
                for i1 in r:
                    idx2[i1] = -1; nm -= 1
    return nm, idx2, st


# ---- the oracle, target by target
def oracle_row(oracle, cur, tgt, nnratio=0.9, check_ori=True):
    """(nmatches, matches12[n1] = the target's map-point ids) of oracle.search_by_bow_kf_kf on this pair alone."""
    return oracle.search_by_bow_kf_kf(cur["kps"], cur["desc"], cur["mp"], cur["bad"], cur["fv"], tgt["kps"], tgt["desc"], tgt["mp"], tgt["bad"], tgt["fv"],
                                      nnratio, check_ori)


def oracle_rows(oracle, cur, targets, nnratio=0.9, check_ori=True):
    ids = np.full((len(targets), len(cur["desc"])), -1, np.int32); nm = np.zeros(len(targets), np.int32)
    for t, tgt in enumerate(targets):
        nm[t], ids[t] = oracle_row(oracle, cur, tgt, nnratio, check_ori)
    return ids, nm


def ids_of(targets, idx2):
    """match_idx2 rows -> the map-point ids the oracle reports (targets[t].mp[match_idx2])."""
    out = np.full(idx2.shape, -1, np.int32)
    for t, tgt in enumerate(targets):
        m = idx2[t] >= 0
        out[t][m] = tgt["mp"][idx2[t][m]]
    return out
