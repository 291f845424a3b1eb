"""GPU parity of the grid build and the searches on top of it at the sizes the ABI admits but no other test reaches: 2 049 to 8 192
keypoints per slot, where frame_build_block sorts P = 4 096 or 8 192 keys (4 or 8 per thread) and sorted positions, keypoint indices and
slot offsets use their full 13 bits.  Everything is compared bit-exactly with the CPU oracle (oracle.Grid.match_window,
pyoracle.project_search, fuse_targets_scene.oracle_rows).

What a scene has to exercise is asserted on the ORACLE's results alone (the share of self hits, of winners from the upper half of the index
range, the accepted counts, the ranked walks reaching depth 3), so a scene that stops reaching the large sizes fails instead of passing by."""
import functools

import numpy as np
import pytest

import fuse_targets_scene as fts
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CAP = 8192
DEFAULT = (0.0, 640.0, 0.0, 480.0)
UNDISTORTED = (-12.5, 655.25, -7.75, 489.5)          # undistorted-image style: negative, non-integer minima
SIZES = (2048, 2049, 4095, 4096, 4097, 8191, 8192)
# every n with the uniform layout at the default bounds, one capacity that is no power of two and smaller than P; the other layouts and
# the second set of bounds at 4 097 (P = 8 192, half of it padding) and 8 192 (no padding at all)
CASES = [(CAP, n, "uniform", DEFAULT) for n in SIZES] + [(5000, 5000, "uniform", DEFAULT)]
CASES += [(CAP, n, layout, bounds) for n in (4097, 8192) for layout, bounds in (
    ("none_inside", DEFAULT), ("one_cell", DEFAULT), ("one_column", DEFAULT), ("one_row", DEFAULT), ("integer", DEFAULT),
    ("uniform", UNDISTORTED), ("integer", UNDISTORTED))]
# layouts whose cells hold a few keypoints each: the first candidate in (column, row, index) order then has any index.  Inside a cell the
# order IS the index order, so where a cell holds hundreds of keypoints (one cell, one column, one row: measured 0.0 - 0.3 % of winners from
# the upper half) a tie goes to one of the cell's first few; with none inside there is no winner.
SPREAD = ("uniform", "integer")
UPPER_SHARE = 0.20
FIELDS = ("best_idx", "best_dist", "second_dist", "best_level", "second_level")
BASE = np.random.default_rng(4242).integers(0, 256, (4, 32), dtype=np.uint8)      # the 4 descriptors of the tie grids and tie queries
NQ = 2000


def _case_id(c):
    cap, n, layout, bounds = c
    return f"{layout}-{'default' if bounds is DEFAULT else 'undistorted'}-n{n}" + ("" if cap == CAP else f"-cap{cap}")


case_params = pytest.mark.parametrize("case", CASES, ids=_case_id)


def _check_matches(g, o):
    for k in FIELDS:
        assert np.array_equal(g[k].astype(np.int64), o[k].astype(np.int64)), k


def _check_nothing(m):
    assert np.all(m["best_idx"] == -1) and np.all(m["best_dist"] == 256) and np.all(m["second_dist"] == 256)
    assert np.all(m["best_level"] == -1) and np.all(m["second_level"] == -1)


class _Scene:
    pass


def _upper_share(o, n):
    return float((o["best_idx"] >= n / 2).mean())


@functools.lru_cache(maxsize=None)
def _scene(n, layout, bounds=DEFAULT):
    """n keypoints in `layout`, one set of unique descriptors and one of only 4 distinct values, the oracle's grid.  Never modified.
    A fifth of the tie queries has r = 700 and is won by the first keypoint in grid order that carries the query's descriptor: four
    keypoints decide 20 % of the winners, so the upper-half share of a random scene lies anywhere between about 20 and 40 %.  The scene is the
    first of a fixed sequence whose ORACLE result meets the share the test asserts (the test still asserts it)."""
    for salt in range(8):
        s = _make_scene(n, layout, bounds, salt)
        if not (n >= 4096 and layout in SPREAD) or _upper_share(_oracle_ties_of(s, "plain"), n) >= UPPER_SHARE:
            break
    return s


def _make_scene(n, layout, bounds, salt):
    rng = np.random.default_rng([n, sorted(("uniform", "none_inside", "one_cell", "one_column", "one_row", "integer")).index(layout),
                                 int(bounds is not DEFAULT), salt])
    s = _Scene()
    s.n, s.layout, s.bounds = n, layout, bounds
    kps = np.zeros(n, po.KP_DTYPE)
    if layout == "uniform":              # some keypoints fall outside the grid (PosInGrid drops them)
        x, y = rng.uniform(-5, 645, n), rng.uniform(-5, 485, n)
    elif layout == "none_inside":        # right of and below the grid, and left of / above it: n_sorted = 0
        x, y = rng.uniform(700, 900, n), rng.uniform(-300, 800, n)
        x[::2] = rng.uniform(-300, -40, len(x[::2]))
    elif layout == "one_cell":           # grid cell (30, 20) of the default bounds: x in [295, 305), y in [195, 205)
        x, y = rng.uniform(296, 304, n), rng.uniform(196, 204, n)
    elif layout == "one_column":
        x, y = np.full(n, 317.25), rng.uniform(-5, 485, n)
    elif layout == "one_row":
        x, y = rng.uniform(-5, 645, n), np.full(n, 201.75)
    else:                                # level-0 keypoints: many (x - minX) * wInv end in .5 and go through roundf
        x, y = rng.integers(0, 640, n), rng.integers(0, 480, n)
    kps["x"], kps["y"] = x.astype(np.float32), y.astype(np.float32)
    kps["octave"] = rng.integers(0, 8, n)
    s.kps = kps
    s.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    assert len(np.unique(s.desc, axis=0)) == n
    s.tie_desc = BASE[rng.integers(0, 4, n)]
    s.skip = (rng.random(n) < 0.3).astype(np.uint8)
    s.grid = po.Grid(kps, *bounds)
    s.ties = {}
    return s


@functools.lru_cache(maxsize=None)
def _tie_queries():
    """(qdesc, qx, qy, qr, unbounded levels, random qmin, random qmax): 2 000 queries with the grids' 4 descriptors."""
    rng = np.random.default_rng(99)
    qd = BASE[rng.integers(0, 4, NQ)]
    qx = rng.uniform(0, 640, NQ).astype(np.float32)
    qy = rng.uniform(0, 480, NQ).astype(np.float32)
    qr = rng.choice([0, 0.5, 20, 60, 700], NQ).astype(np.float32)
    neg = np.full(NQ, -1, np.int32)
    return qd, qx, qy, qr, neg, rng.integers(-1, 8, NQ).astype(np.int32), rng.integers(-1, 8, NQ).astype(np.int32)


def _oracle_ties_of(s, mode):
    """The oracle's answer to the tie queries on the scene's tie grid, computed once.  mode: plain / skip / levels."""
    if mode not in s.ties:
        qd, qx, qy, qr, neg, lmin, lmax = _tie_queries()
        qmin, qmax = (lmin, lmax) if mode == "levels" else (neg, neg)
        s.ties[mode] = s.grid.match_window(s.tie_desc, qd, qx, qy, qr, qmin, qmax, skip=s.skip if mode == "skip" else None)
    return s.ties[mode]


def _oracle_ties(n, layout, bounds, mode):
    return _oracle_ties_of(_scene(n, layout, bounds), mode)


def _built(capi, cap, s, desc):
    g = capi.FrameGrid(capacity=cap)
    g.build(s.kps, desc, s.bounds)
    return g


@case_params
def test_self_queries(capi, case):
    """Query i = keypoint i's position and (unique) descriptor, r = 0.5: every indexed keypoint is reachable from its own window."""
    cap, n, layout, bounds = case
    s = _scene(n, layout, bounds)
    half = np.full(n, 0.5, np.float32)
    neg = np.full(n, -1, np.int32)
    o = s.grid.match_window(s.desc, s.desc, s.kps["x"], s.kps["y"], half, neg, neg)
    hits = float((o["best_idx"] == np.arange(n)).mean())
    print(f"self hits {hits:.4f}")
    if layout == "uniform":
        assert hits >= 0.95                        # the rest lies outside the grid
    g = _built(capi, cap, s, s.desc)
    try:
        got = g.match_window(s.desc, s.kps["x"], s.kps["y"], half, neg, neg)
        _check_matches(got, o)
        if layout == "none_inside":
            _check_nothing(got)
        # r = 0 on top of a keypoint with its own descriptor: |dx| < r is strict, so there is no candidate
        zero = np.zeros(n, np.float32)
        got0 = g.match_window(s.desc, s.kps["x"], s.kps["y"], zero, neg, neg)
        _check_nothing(got0)
        _check_matches(got0, s.grid.match_window(s.desc, s.desc, s.kps["x"], s.kps["y"], zero, neg, neg))
    finally:
        g.close()


@case_params
def test_tie_queries(capi, case):
    """Only 4 distinct descriptors: the winner is the first candidate in (column, row, index) order, also among sorted positions and
    indices above 2 048 -- plain, with a skip mask of density 0.3 and with random level ranges."""
    cap, n, layout, bounds = case
    s = _scene(n, layout, bounds)
    qd, qx, qy, qr, neg, lmin, lmax = _tie_queries()
    o = _oracle_ties(n, layout, bounds, "plain")
    upper = _upper_share(o, n)
    print(f"winners from the upper half of the index range {upper:.4f}, queries with a winner {float((o['best_idx'] >= 0).mean()):.4f}")
    if n >= 4096 and layout in SPREAD:
        assert upper >= UPPER_SHARE
    g = _built(capi, cap, s, s.tie_desc)
    try:
        got = g.match_window(qd, qx, qy, qr, neg, neg)
        _check_matches(got, o)
        _check_nothing(got[qr == 0])
        _check_matches(g.match_window(qd, qx, qy, qr, neg, neg, skip=s.skip), _oracle_ties(n, layout, bounds, "skip"))
        _check_matches(g.match_window(qd, qx, qy, qr, lmin, lmax), _oracle_ties(n, layout, bounds, "levels"))
        if layout == "none_inside":
            _check_nothing(got)
            _check_nothing(g.match_window(qd, qx, qy, qr, lmin, lmax, skip=s.skip))
    finally:
        g.close()


@case_params
def test_top2_and_ranked(capi, case):
    """dvm_match_window_top2's runner-up and dvm_match_window_ranked's list of four on the tie grid: entry c is what the oracle's scan
    returns with entries 0..c-1 masked as well."""
    cap, n, layout, bounds = case
    s = _scene(n, layout, bounds)
    qd, qx, qy, qr, neg, _, _ = _tie_queries()
    o = _oracle_ties(n, layout, bounds, "skip")
    g = _built(capi, cap, s, s.tie_desc)
    try:
        g2, second = g.match_window(qd, qx, qy, qr, neg, neg, skip=s.skip, top2=True)
        ridx, rdist = g.match_window_ranked(qd, qx, qy, qr, neg, neg, skip=s.skip)
    finally:
        g.close()
    _check_matches(g2, o)
    assert np.all((second >= 0) == (o["second_dist"] < 256))
    assert np.array_equal(ridx[:, 0], o["best_idx"]) and np.array_equal(rdist[:, 0], o["best_dist"])
    assert np.array_equal(ridx[:, 1], second) and np.array_equal(rdist[:, 1], o["second_dist"])
    assert np.all(rdist[ridx < 0] == 256) and ridx.max() < n
    deep = 0
    for q in np.flatnonzero(o["second_dist"] < 256)[:100]:
        sk = s.skip.copy()
        for c in range(4):
            w = s.grid.match_window(s.tie_desc, qd[q:q + 1], qx[q:q + 1], qy[q:q + 1], qr[q:q + 1], neg[:1], neg[:1], skip=sk)
            assert int(w["best_idx"][0]) == int(ridx[q, c]), (q, c)
            if w["best_idx"][0] < 0:
                assert np.all(ridx[q, c:] < 0) and np.all(rdist[q, c:] == 256)
                break
            assert int(w["best_dist"][0]) == int(rdist[q, c]), (q, c)
            sk[w["best_idx"][0]] = 1
            deep += c == 3
    print(f"ranked walks reaching depth 3: {deep}")
    if layout == "none_inside":
        assert np.all(ridx == -1) and np.all(rdist == 256) and np.all(second == -1)
    else:
        assert deep > 20


def test_slots_and_rebuilds(capi):
    """Three slots of 8 192 built from device arrays with counts [8192, 0, 4097], then rebuilt with [100, 8192, 0] from other keypoints:
    slot addressing at the full capacity, and a slot that shrank (or grew) behaves as a fresh grid -- nothing of the stale skp / sidx /
    sdesc / cellx_start of the earlier build shows."""
    import torch
    qd, qx, qy, qr, neg, _, _ = _tie_queries()
    filler = _scene(CAP, "one_row")                  # rows past a slot's count hold real-looking keypoints: reading them would show
    g = capi.FrameGrid(capacity=CAP, slots=3)

    def build_and_compare(scenes):
        K = np.tile(filler.kps, (3, 1))
        D = np.tile(filler.tie_desc, (3, 1, 1))
        for slot, s in enumerate(scenes):
            if s is not None:
                K[slot, :s.n], D[slot, :s.n] = s.kps, s.tie_desc
        d_k = torch.from_numpy(K.view(np.uint8).reshape(-1).copy()).cuda()
        d_d = torch.from_numpy(D.reshape(-1).copy()).cuda()
        d_n = torch.tensor([0 if s is None else s.n for s in scenes], dtype=torch.int32).cuda()
        g.build_batch_device(0, 3, d_k.data_ptr(), CAP, d_d.data_ptr(), CAP * 32, d_n.data_ptr(), DEFAULT)
        torch.cuda.synchronize()
        assert g.overflows() == 0
        for slot, s in enumerate(scenes):
            for skip in (None, np.zeros(0, np.uint8) if s is None else s.skip):
                got = g.match_window(qd, qx, qy, qr, neg, neg, skip=skip, slot=slot)
                ridx, rdist = g.match_window_ranked(qd, qx, qy, qr, neg, neg, skip=skip, slot=slot)
                if s is None:
                    _check_nothing(got)
                    assert np.all(ridx == -1) and np.all(rdist == 256)
                    continue
                o = _oracle_ties(s.n, s.layout, s.bounds, "plain" if skip is None else "skip")
                _check_matches(got, o)
                assert np.array_equal(ridx[:, 0], o["best_idx"]) and np.array_equal(rdist[:, 0], o["best_dist"])
                assert np.array_equal(rdist[:, 1], o["second_dist"]) and np.all(rdist[ridx < 0] == 256)
                assert (o["best_idx"] >= 0).mean() > 0.2       # (the slot's queries do find something)

    try:
        build_and_compare([_scene(8192, "uniform"), None, _scene(4097, "uniform")])
        build_and_compare([_scene(100, "uniform"), _scene(8192, "integer"), None])
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------- projection searches on large grids
@functools.lru_cache(maxsize=None)
def _fuse_scene(N):
    """fts.scene(2, 2, n_keypoints=N), first 200 points, with each target's keypoint rows permuted: the scene puts the true projections in a
    target's first rows, so without the permutation every accepted index is below 2 048."""
    sc = fts.prefix(fts.scene(2, 2, n_keypoints=N), 200)
    perm = np.random.default_rng(1234).permutation(N)
    targets = [dict(kf, kps=kf["kps"][perm].copy(), desc=np.ascontiguousarray(kf["desc"][perm]), pt_of_kp=kf["pt_of_kp"][perm]) for kf in sc["targets"]]
    return dict(targets=targets, pts=sc["pts"], skip=sc["skip"])


def _no_valid(pts):
    return {k: v for k, v in pts.items() if k != "valid"}


@functools.lru_cache(maxsize=None)
def _oracle_fuse_rows(N, masked):
    sc = _fuse_scene(N)
    return fts.oracle_rows(sc["targets"], sc["pts"], sc["skip"] if masked else None, masked)


def _check_fuse_scene(N):
    """On the oracle alone: enough accepted entries, and a quarter of them among the upper half of the keypoint indices."""
    bi, _ = _oracle_fuse_rows(N, False)
    acc = bi[bi >= 0]
    print(f"N = {N}: accepted {len(acc)}, of them with index >= N / 2: {float((acc >= N / 2).mean()):.4f}; masked run {(_oracle_fuse_rows(N, True)[0] >= 0).sum()}")
    assert len(acc) >= 0.25 * 2 * 200 * 0.8
    assert (acc >= N / 2).mean() >= 0.25


@functools.lru_cache(maxsize=None)
def _oracle_project(N, t, gate):
    """pyoracle.project_search of the 200 points on target t: (best_idx, best_dist, second_dist).  The oracle reports no second distance;
    it is the best distance of the same search with the winner's keypoint masked."""
    sc = _fuse_scene(N)
    kf, pts = sc["targets"][t], _no_valid(sc["pts"])
    bi, bd, _ = fts.oracle_target(kf, pts, np.ones(200, np.uint8), 3.0, gate)
    sd = np.full(200, 256, np.int32)
    for i in np.flatnonzero(bi >= 0):
        one = {k: v[i:i + 1] for k, v in pts.items()}
        one["valid"] = np.ones(1, np.uint8)
        mask = np.zeros(N, np.uint8); mask[bi[i]] = 1
        sd[i] = po.project_search(kf["kps"], kf["desc"], kf["bounds"], mask, kf["Tcw"], po.se3_inverse(kf["Tcw"])[4:], kf["K"], one, 3.0,
                                  kf["scale_factors"], kf["log_scale_factor"], kf["inv_level_sigma2"] if gate else None, 5.99)[1][0]
    return bi, bd, sd


@pytest.mark.parametrize("gate", [True, False], ids=("gate5.99", "no_gate"))
@pytest.mark.parametrize("N", [4097, 8192])
def test_project_search_large_grid(capi, N, gate):
    _check_fuse_scene(N)
    sc = _fuse_scene(N)
    pts = _no_valid(sc["pts"])
    for t, kf in enumerate(sc["targets"]):
        bi, bd, sd = _oracle_project(N, t, gate)
        assert (bi >= N / 2).sum() >= 10
        g = capi.FrameGrid(CAP)
        try:
            g.build(kf["kps"], kf["desc"], tuple(float(x) for x in kf["bounds"]))
            cam = dict(Tcw=kf["Tcw"], Ow=capi.se3_inverse(kf["Tcw"])[4:], K=kf["K"], bounds=kf["bounds"], log_scale_factor=kf["log_scale_factor"])
            m, _ = capi.project_search(g, cam, pts, 3.0, kf["scale_factors"], gate_inv_sigma2=kf["inv_level_sigma2"] if gate else None, gate=5.99)
        finally:
            g.close()
        assert np.array_equal(m["best_idx"], bi) and np.array_equal(m["best_dist"], bd) and np.array_equal(m["second_dist"], sd)


@pytest.mark.parametrize("N", [4097, 8192])
def test_fuse_targets_large_targets(capi, N):
    _check_fuse_scene(N)
    sc = _fuse_scene(N)
    h = capi.FuseTargets()
    try:
        h.reserve(200, 2, 2 * 8192)
        h.set(sc["targets"])
        bi, bd = h.run(_no_valid(sc["pts"]), 3.0, None)
        want = _oracle_fuse_rows(N, False)
        assert np.array_equal(bi, want[0]) and np.array_equal(bd, want[1])
        bi, bd = h.run(sc["pts"], 3.0, sc["skip"])
        want = _oracle_fuse_rows(N, True)
        assert np.array_equal(bi, want[0]) and np.array_equal(bd, want[1])
        assert (want[0] >= 0).sum() >= 0.25 * 2 * 200 * 0.6
    finally:
        h.close()


def test_fuse_targets_refuses_8193_keypoints(capi):
    sc = _fuse_scene(8192)
    h = capi.FuseTargets()
    try:
        h.reserve(200, 2, 2 * 8192)
        h.set(sc["targets"])
        n = 8193
        with pytest.raises(capi.DvmError) as e:
            h.set([sc["targets"][0], dict(sc["targets"][1], kps=np.zeros(n, capi.KP_DTYPE), desc=np.zeros((n, 32), np.uint8))])
        assert e.value.code == -1 and "n outside [0, 8192]" in str(e.value)
        bi, bd = h.run(sc["pts"], 3.0, sc["skip"])                # the resident targets of 8 192 still serve
        want = _oracle_fuse_rows(8192, True)
        assert np.array_equal(bi, want[0]) and np.array_equal(bd, want[1])
    finally:
        h.close()
