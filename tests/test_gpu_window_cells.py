"""The window searches scan the cells of the query's rectangle only (FrameView::cell_start, window_scan of csrc/match_device.h): every
kernel that calls the scan, bit for bit against oracle.pyoracle (Grid.match_window, project_search, search_by_projection_frames), and
dvm_orb_copy_result as one launch.

Two scenes of 300 keypoints on bounds (0, 640, 0, 480), octaves 0 - 7: `sparse` (most cells empty, some keypoints outside the grid) and
`dense` (100 keypoints in each of the cells (30, 20), (30, 21), (31, 20): spans longer than a DPP row and than a wave, in one column and in
two adjacent ones).  Each with unique descriptors and with descriptors drawn from four (ties, settled by scan position).  519 queries: 512
random ones with radii from 0 to 700 and seven placed by hand (1, 2, 16, 17 columns; corners).  `reference` asserts, from the rectangle
formula and the oracle's answers alone, that the scenes reach the paths they are for."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

SEED = 2407
N_KP, N_RANDOM = 300, 512
BOUNDS = (0.0, 640.0, 0.0, 480.0)
RADII = (0, 0.5, 7, 20, 60, 170, 700)
PLACED = ((325, 240, 75), (320, 240, 75), (325, 240, 80), (5, 240, 155), (635, 5, 155), (320, 240, 0), (322, 240, 0.5))
DENSE_CELLS = ((30, 20), (30, 21), (31, 20))
SF = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
LOG_SF = float(np.log(np.float32(1.2)))
F = np.float32
MATCH_FIELDS = ("best_idx", "best_dist", "second_dist", "best_level", "second_level")


@functools.lru_cache(maxsize=None)
def scene(kind):
    """dict(kps, desc_unique, desc_ties, base): the keypoints of `kind` and its two descriptor sets."""
    rng = np.random.default_rng(SEED + (0 if kind == "sparse" else 1))
    kps = np.zeros(N_KP, po.KP_DTYPE)
    if kind == "sparse":
        kps["x"] = rng.uniform(-5, 645, N_KP); kps["y"] = rng.uniform(-5, 485, N_KP)
    else:   # PosInGrid rounds: cell (cx, cy) holds x in [10 cx - 5, 10 cx + 5)
        for i, (cx, cy) in enumerate(DENSE_CELLS):
            kps["x"][100 * i:100 * i + 100] = 10 * cx + rng.uniform(-4.5, 4.5, 100); kps["y"][100 * i:100 * i + 100] = 10 * cy + rng.uniform(-4.5, 4.5, 100)
    kps["octave"] = rng.integers(0, 8, N_KP)
    kps["angle"] = rng.uniform(0, 360, N_KP); kps["size"] = 31.0 * SF[kps["octave"]]
    base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    return dict(kps=kps, desc_unique=rng.integers(0, 256, (N_KP, 32), dtype=np.uint8), desc_ties=base[rng.integers(0, 4, N_KP)], base=base)


@functools.lru_cache(maxsize=None)
def queries(kind, ties):
    """dict(x, y, r, desc, qmin, qmax (random levels), skip (30 % of the keypoints))"""
    sc = scene(kind)
    rng = np.random.default_rng(SEED + 10 + 2 * (kind == "dense") + ties)
    nq = N_RANDOM + len(PLACED)
    x = np.concatenate([rng.uniform(-30, 670, N_RANDOM), [p[0] for p in PLACED]]).astype(F)
    y = np.concatenate([rng.uniform(-30, 510, N_RANDOM), [p[1] for p in PLACED]]).astype(F)
    r = np.concatenate([rng.choice(RADII, N_RANDOM), [p[2] for p in PLACED]]).astype(F)
    if ties:
        desc = sc["base"][rng.integers(0, 4, nq)]
    else:       # a keypoint's descriptor with a few bits flipped: a clear winner where that keypoint is in the window
        desc = sc["desc_unique"][rng.integers(0, N_KP, nq)].copy()
        desc[np.arange(nq), rng.integers(0, 32, nq)] ^= rng.integers(1, 256, nq).astype(np.uint8)
    return dict(x=x, y=y, r=r, desc=np.ascontiguousarray(desc), qmin=rng.integers(-1, 8, nq).astype(np.int32), qmax=rng.integers(-1, 8, nq).astype(np.int32),
                skip=(rng.random(N_KP) < 0.3).astype(np.uint8))


def rectangle(x, y, r):
    """Frame::GetFeaturesInArea's cell rectangle in float32 (x0, x1, y0, y1 arrays) and whether it is empty."""
    inv = F(64) / F(640), F(48) / F(480)
    x0 = np.maximum(0, np.floor((x - F(0) - r) * inv[0]).astype(np.int64)); x1 = np.minimum(63, np.ceil((x - F(0) + r) * inv[0]).astype(np.int64))
    y0 = np.maximum(0, np.floor((y - F(0) - r) * inv[1]).astype(np.int64)); y1 = np.minimum(47, np.ceil((y - F(0) + r) * inv[1]).astype(np.int64))
    empty = (x0 >= 64) | (x1 < 0) | (y0 >= 48) | (y1 < 0)
    return x0, x1, y0, y1, empty


def _desc(kind, ties):
    return scene(kind)["desc_ties" if ties else "desc_unique"]


@functools.lru_cache(maxsize=None)
def oracle_match(kind, ties, mode):
    """Grid.match_window of the oracle: mode plain | skip | levels"""
    sc, q = scene(kind), queries(kind, ties)
    neg = np.full(len(q["x"]), -1, np.int32)
    qmin, qmax = (q["qmin"], q["qmax"]) if mode == "levels" else (neg, neg)
    return po.Grid(sc["kps"], *BOUNDS).match_window(_desc(kind, ties), q["desc"], q["x"], q["y"], q["r"], qmin, qmax, skip=q["skip"] if mode == "skip" else None)


@pytest.fixture(scope="module")
def reference():
    """The shares the scenes are built for, from the rectangle formula and the oracle alone (seed 2407, sparse / dense: more than 16 columns 0.29 / 0.31,
    all 64 columns 0.14 / 0.16, empty 0.075 / 0.081, winners on the tie descriptors 0.53 / 0.21, of which tied 0.73 / 1.0)."""
    out = {}
    for kind in ("sparse", "dense"):
        q = queries(kind, True)
        x0, x1, _, _, empty = rectangle(q["x"], q["y"], q["r"])
        cols = (x1 - x0 + 1)[~empty]
        assert {1, 2, 16, 17, 64} <= set(cols.tolist()) and ((cols >= 33) & (cols <= 63)).any()
        m = oracle_match(kind, True, "plain")
        win = m["best_idx"] >= 0
        out[kind] = dict(over16=(cols > 16).mean(), all64=(cols == 64).mean(), empty=empty.mean(), winners=win.mean(),
                         tied=(m["second_dist"][win] == m["best_dist"][win]).mean())
        assert out[kind]["over16"] >= 0.2 and out[kind]["all64"] >= 0.1 and out[kind]["empty"] >= 0.02, out[kind]
    assert out["sparse"]["winners"] >= 0.4 and out["dense"]["winners"] >= 0.15 and out["sparse"]["tied"] >= 0.5, out
    return out


def _same(got, want, fields=MATCH_FIELDS):
    for k in fields:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), k


def _grid(capi, kind, ties, **kw):
    g = capi.FrameGrid(capacity=2048, **kw)
    g.build(scene(kind)["kps"], _desc(kind, ties), BOUNDS)
    return g


@pytest.mark.parametrize("ties", [False, True], ids=("unique", "ties"))
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_match_window_top2(capi, reference, kind, ties):
    q = queries(kind, ties)
    neg = np.full(len(q["x"]), -1, np.int32)
    g = _grid(capi, kind, ties)
    _same(g.match_window(q["desc"], q["x"], q["y"], q["r"], neg, neg), oracle_match(kind, ties, "plain"))
    _same(g.match_window(q["desc"], q["x"], q["y"], q["r"], neg, neg, skip=q["skip"]), oracle_match(kind, ties, "skip"))
    _same(g.match_window(q["desc"], q["x"], q["y"], q["r"], q["qmin"], q["qmax"]), oracle_match(kind, ties, "levels"))
    # the runner-up's index: what the oracle finds with the winner masked as well
    m, second = g.match_window(q["desc"], q["x"], q["y"], q["r"], neg, neg, top2=True)
    _same(m, oracle_match(kind, ties, "plain"))
    assert np.array_equal(second >= 0, m["second_dist"] < 256)
    go = po.Grid(scene(kind)["kps"], *BOUNDS)
    for i in np.flatnonzero(second >= 0)[:60]:
        mask = np.zeros(N_KP, np.uint8); mask[m["best_idx"][i]] = 1
        o = go.match_window(_desc(kind, ties), q["desc"][i:i + 1], q["x"][i:i + 1], q["y"][i:i + 1], q["r"][i:i + 1], neg[:1], neg[:1], skip=mask)
        assert (int(o["best_idx"][0]), int(o["best_dist"][0])) == (int(second[i]), int(m["second_dist"][i]))
    g.close()


@pytest.mark.parametrize("ties", [False, True], ids=("unique", "ties"))
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_ranked_search(capi, reference, kind, ties):
    """Entry c of the ranked list is the oracle's winner with entries 0 .. c-1 masked."""
    q = queries(kind, ties)
    nq = len(q["x"])
    g = _grid(capi, kind, ties)
    idx, dist = g.match_window_ranked(q["desc"], q["x"], q["y"], q["r"], q["qmin"], q["qmax"], skip=q["skip"])
    g.close()
    go = po.Grid(scene(kind)["kps"], *BOUNDS)
    _same(dict(best_idx=idx[:, 0], best_dist=dist[:, 0]), go.match_window(_desc(kind, ties), q["desc"], q["x"], q["y"], q["r"], q["qmin"], q["qmax"], skip=q["skip"]),
          ("best_idx", "best_dist"))
    deep = 0
    for i in np.flatnonzero(idx[:, 1] >= 0)[::3]:
        mask = q["skip"].copy()
        for c in range(4):
            o = go.match_window(_desc(kind, ties), q["desc"][i:i + 1], q["x"][i:i + 1], q["y"][i:i + 1], q["r"][i:i + 1], q["qmin"][i:i + 1], q["qmax"][i:i + 1], skip=mask)
            assert (int(o["best_idx"][0]), int(o["best_dist"][0])) == (int(idx[i, c]), int(dist[i, c])), (i, c)
            if idx[i, c] < 0:
                assert np.all(idx[i, c:] < 0) and np.all(dist[i, c:] == 256)
                break
            mask[idx[i, c]] = 1
            deep += c == 3
    assert deep >= 10 and nq == N_RANDOM + len(PLACED)


@pytest.mark.parametrize("ties", [False, True], ids=("unique", "ties"))
def test_match_frames_batch(capi, reference, ties):
    """Frame-to-frame search on the device: the queries are keypoints (window 15 * scale[octave], octaves o - 1 .. o + 1).  A handle of six
    slots, the batch in slots 3 .. 5 (its last), pair 0 from a carry frame: carry -> sparse, sparse -> dense, dense -> sparse."""
    import torch
    order = ("sparse", "dense", "sparse")
    cap = 320
    carry = scene("dense")
    kps = np.zeros((3, cap), capi.KP_DTYPE); desc = np.zeros((3, cap, 32), np.uint8)
    for s, kind in enumerate(order):
        kps[s, :N_KP] = scene(kind)["kps"]; desc[s, :N_KP] = _desc(kind, ties)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    d_k, d_d, d_n = dev(kps), dev(desc), torch.tensor([N_KP] * 3, dtype=torch.int32).cuda()
    c_k, c_d, c_n = dev(carry["kps"]), dev(_desc("dense", ties)), torch.tensor([N_KP], dtype=torch.int32).cuda()
    d_sf = torch.from_numpy(SF).cuda()
    g = capi.FrameGrid(capacity=cap, slots=6)
    g.build_batch_device(3, 3, d_k.data_ptr(), cap, d_d.data_ptr(), cap * 32, d_n.data_ptr(), BOUNDS)
    out = torch.zeros((3, cap, 4), dtype=torch.int32, device="cuda"); nq = torch.zeros(3, dtype=torch.int32, device="cuda")
    g.match_frames_batch(3, 3, d_k.data_ptr(), cap, d_d.data_ptr(), cap * 32, d_n.data_ptr(), (c_k.data_ptr(), c_d.data_ptr(), c_n.data_ptr()), cap, 15.0,
                         d_sf.data_ptr(), 8, out.data_ptr(), cap, nq.data_ptr())
    torch.cuda.synchronize()
    res = out.cpu().numpy().view(capi.MATCH_DTYPE).reshape(3, cap)
    assert nq.cpu().tolist() == [N_KP] * 3
    found = 0
    for s, kind in enumerate(order):
        qk, qd = (carry["kps"], _desc("dense", ties)) if s == 0 else (scene(order[s - 1])["kps"], _desc(order[s - 1], ties))
        ref = po.Grid(scene(kind)["kps"], *BOUNDS).match_window(_desc(kind, ties), qd, qk["x"], qk["y"], (F(15) * SF[qk["octave"]]).astype(F), qk["octave"] - 1,
                                                                   qk["octave"] + 1)
        _same(res[s][:N_KP], ref)
        found += int((ref["best_idx"] >= 0).sum())
    assert found >= 100
    g.close()


def _points_at(q, rng, lvl=None):
    """Map points that an identity camera (fx = fy = 500, c = (320, 240)) projects onto the queries (x, y, desc), predicted at level lvl
    (random without one): dict for project_search / the fuse chain."""
    n = len(q["x"])
    z = rng.uniform(4, 8, n)
    pos = np.column_stack([(q["x"] - 320.0) / 500.0 * z, (q["y"] - 240.0) / 500.0 * z, z]).astype(F)
    dist = np.linalg.norm(pos.astype(np.float64), axis=1)
    lvl = rng.integers(0, 8, n) if lvl is None else lvl
    max_dist = (dist * SF[lvl] * rng.uniform(0.9, 1.0, n)).astype(F)              # PredictScale then gives a level near lvl
    normal = (pos / np.linalg.norm(pos, axis=1, keepdims=True)).astype(F)
    return dict(pos=pos, normal=normal, min_dist=(max_dist / SF[7] * F(0.5)).astype(F), max_dist=max_dist, desc=q["desc"],
                valid=(rng.random(n) < 0.9).astype(np.uint8))


IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
K4 = np.array([500.0, 500.0, 320.0, 240.0], np.float32)


def _keyframe(kind, ties):
    return dict(kps=scene(kind)["kps"], desc=_desc(kind, ties), Tcw=IDENTITY, K=K4, bounds=np.array(BOUNDS, np.float32), scale_factors=SF,
                level_sigma2=(SF * SF).astype(F), inv_level_sigma2=(F(1) / (SF * SF)).astype(F), log_scale_factor=LOG_SF)


@pytest.mark.parametrize("th", [0.4, 6.0, 48.0, 200.0])
@pytest.mark.parametrize("ties", [False, True], ids=("unique", "ties"))
@pytest.mark.parametrize("kind", ["sparse", "dense"])
def test_project_search_pinhole(capi, reference, kind, ties, th):
    """dvm_project_search: radius th * scale[level] from 0.4 to 717 px, levels [l - 1, l], with and without skip flags."""
    q, kf = queries(kind, ties), _keyframe(kind, ties)
    pts = _points_at(q, np.random.default_rng(SEED + 20))
    Ow = po.se3_inverse(IDENTITY)[4:]
    g = _grid(capi, kind, ties)
    cam = dict(Tcw=IDENTITY, Ow=capi.se3_inverse(IDENTITY)[4:], K=K4, bounds=kf["bounds"], log_scale_factor=LOG_SF)
    hits = 0
    for skip in (None, q["skip"]):
        bi, bd, pr = po.project_search(kf["kps"], kf["desc"], kf["bounds"], skip, IDENTITY, Ow, K4, pts, th, SF, LOG_SF)
        m, proj = capi.project_search(g, cam, pts, th, SF, skip=skip, gate_inv_sigma2=None, valid=pts["valid"])
        assert np.array_equal(proj["level"], pr[:, 3].astype(np.int32))
        assert np.array_equal(m["best_idx"], bi) and np.array_equal(m["best_dist"], bd)
        hits += int((bi >= 0).sum())
    assert (pr[:, 3] >= 0).mean() > 0.5 and (hits > 0 or th < 1)
    g.close()


@pytest.mark.parametrize("ties", [False, True], ids=("unique", "ties"))
def test_fuse_chain_two_targets(capi, reference, ties):
    """dvm_fuse_targets with the two scenes as its targets (grids carved from the chain's own block, k_ft_build / k_ft_search), th from a
    3-px window to one over the whole image (the 5.99 gate then drops what is far: the scan still walks the rectangle)."""
    h = capi.FuseTargets()
    h.reserve(N_RANDOM + len(PLACED) + 2 * N_KP, 2, 2 * N_KP)
    targets = [_keyframe("sparse", ties), _keyframe("dense", ties)]
    h.set(targets)
    # the queries, and behind them points on the keypoints of both scenes at the keypoints' own levels: those pass the gate
    q, on = queries("dense", ties), [scene(k)["kps"] for k in ("sparse", "dense")]
    q = dict(x=np.concatenate([q["x"]] + [k["x"] for k in on]), y=np.concatenate([q["y"]] + [k["y"] for k in on]),
             desc=np.concatenate([q["desc"], _desc("sparse", ties), _desc("dense", ties)]))
    n_q = len(q["x"]) - 2 * N_KP
    rng = np.random.default_rng(SEED + 21)
    pts = _points_at(q, rng, np.concatenate([rng.integers(0, 8, n_q)] + [k["octave"] for k in on]))
    skip = (np.random.default_rng(SEED + 22).random((2, len(q["x"]))) < 0.2).astype(np.uint8)
    Ow = po.se3_inverse(IDENTITY)[4:]
    accepted = 0
    for th in (3.0, 48.0, 200.0):
        bi, bd = h.run(pts, th, skip)
        for t, kf in enumerate(targets):
            oi, od, _ = po.project_search(kf["kps"], kf["desc"], kf["bounds"], None, IDENTITY, Ow, K4, dict(pts, valid=pts["valid"] & (1 - skip[t])), th, SF, LOG_SF,
                                          kf["inv_level_sigma2"], 5.99)
            assert np.array_equal(bd[t], od) and np.array_equal(bi[t], np.where((oi >= 0) & (od <= 50), oi, -1)), (th, t)
            accepted += int((bi[t] >= 0).sum())
    assert accepted >= 100
    h.close()


def _oracle_track_requeries(kps_c, desc_c, kps_l, mps, th):
    """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame) query by query with the oracle's grid (identity pose, every map point
    observed): the assignment it ends with (no rotation check) and the number of queries at whose turn the four best candidates of their
    window were all taken by earlier queries -- the queries the device has to search again, since its ranked list ends there."""
    go = po.Grid(kps_c, *BOUNDS)
    n_c = len(kps_c)
    mp_c = np.full(n_c, -1, np.int32)
    claimed = np.zeros(n_c, np.uint8)
    requeries = 0
    for i in range(len(kps_l)):
        X = mps["pos"][i]
        if F(1.0 / np.float64(X[2])) < 0:
            continue
        u = F(F(K4[0] * X[0]) / X[2]) + K4[2]; v = F(F(K4[1] * X[1]) / X[2]) + K4[3]
        if u < BOUNDS[0] or u > BOUNDS[1] or v < BOUNDS[2] or v > BOUNDS[3]:
            continue
        o = int(kps_l["octave"][i])
        args = (desc_c, mps["desc"][i:i + 1], [u], [v], [F(th) * SF[o]], [o - 1], [o + 1])
        mask = np.zeros(n_c, np.uint8)
        top = []
        for _ in range(4):                                       # the window's first four by (distance, scan position)
            m = go.match_window(*args, skip=mask)
            if m["best_idx"][0] < 0:
                break
            top.append(int(m["best_idx"][0])); mask[top[-1]] = 1
        requeries += len(top) == 4 and all(claimed[j] for j in top)
        m = go.match_window(*args, skip=claimed)
        if m["best_idx"][0] >= 0 and m["best_dist"][0] <= 100:
            mp_c[m["best_idx"][0]] = i; claimed[m["best_idx"][0]] = 1
    return mp_c, requeries


def test_tracked_frame_chain_requeries(capi):
    """The tracked-frame chain extracts its own frame, so its grid is the benchmark stream's (about 1 000 keypoints, dense enough that some
    queries find their four ranked candidates taken): k_track_claims searches those windows again with the whole wave (window_scan<64>).
    The oracle side counts those queries; the chain must report that count and the oracle's matches."""
    from dvm_slam_amd import synth
    frames = synth.frame_stream(3)
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    trk = capi.Tracker(ext)
    orc = po.OrbOracle()
    rng = np.random.default_rng(SEED + 30)
    total = 0
    for t in (1, 2):
        n0, k0, d0, _ = orc.extract(frames[t - 1])
        _, k1, d1, _ = orc.extract(frames[t])
        z = rng.uniform(3, 9, n0).astype(F)
        mps = np.zeros(n0, capi.MAP_POINT_DTYPE)
        mps["pos"][:, 0] = (k0["x"] - K4[2]) / K4[0] * z; mps["pos"][:, 1] = (k0["y"] - K4[3]) / K4[1] * z; mps["pos"][:, 2] = z
        mps["desc"] = d0; mps["n_obs"] = 1
        mp_l = np.arange(n0, dtype=np.int32)
        sim_mp, want_rq = _oracle_track_requeries(k1, d1, k0, mps, 15.0)
        # the count stands on the oracle's own search: its assignment without the rotation check is the simulated one
        n_o, mp_o = po.search_by_projection_frames(k1, d1, np.full(len(k1), -1, np.int32), IDENTITY, K4, np.array(BOUNDS, F), tab["scale"], k0, mp_l, None,
                                                   mps.astype(po.MAP_POINT_DTYPE), 15.0, False)
        assert np.array_equal(mp_o, sim_mp) and n_o == (sim_mp >= 0).sum()
        fused = trk.track(frames[t], IDENTITY, K4, np.array(BOUNDS, F), tab["scale"], tab["inv_sigma2"], k0, mp_l, None, mps, th=15.0)
        n_o, _ = po.search_by_projection_frames(k1, d1, np.full(len(k1), -1, np.int32), IDENTITY, K4, np.array(BOUNDS, F), tab["scale"], k0, mp_l, None,
                                                mps.astype(po.MAP_POINT_DTYPE), 15.0, True)
        assert fused["n"] == len(k1) and fused["replayed_on_host"] == 0 and fused["wide_window"] == 0
        assert fused["nmatches_search"] == n_o
        assert fused["n_requeried"] == want_rq, (t, fused["n_requeried"], want_rq)
        total += want_rq
    assert total >= 1
    trk.close(); ext.close()


def test_rebuilt_slot_leaves_no_stale_cells(capi, oracle):
    """One slot built with 300 keypoints, then 7, then none inside the grid: every build writes the whole cell table."""
    rng = np.random.default_rng(SEED + 40)
    q = queries("sparse", False)
    neg = np.full(len(q["x"]), -1, np.int32)
    g = capi.FrameGrid(capacity=2048, slots=2)
    sc = scene("sparse")
    outside = np.zeros(5, po.KP_DTYPE); outside["x"] = 700.0; outside["y"] = rng.uniform(0, 480, 5)
    for kps, desc in ((sc["kps"], sc["desc_unique"]), (sc["kps"][40:47], sc["desc_unique"][40:47]), (outside, sc["desc_unique"][:5])):
        g.build(kps, desc, BOUNDS, slot=1)
        want = po.Grid(kps, *BOUNDS).match_window(desc, q["desc"], q["x"], q["y"], q["r"], neg, neg)
        _same(g.match_window(q["desc"], q["x"], q["y"], q["r"], neg, neg, slot=1), want)
        if len(kps) == 5:
            assert (want["best_idx"] < 0).all()
    g.close()


def test_copy_result_is_the_result_bytes(capi, frames):
    """dvm_orb_copy_result of frame 0 and of the last frame of a batch of five: the bytes of dvm_orb_result_device, rows past the count
    included, into a destination filled with 0xFF."""
    import torch
    imgs = np.stack([frames[i % len(frames)] for i in range(5)])
    e = capi.OrbExtractor(max_batch=5)
    e.extract_batch_host(imgs)
    e.sync()
    for frame in (0, 4):
        k_ptr, d_ptr, n_ptr, cap = e.result_device(frame)
        ksz = capi.KP_DTYPE.itemsize
        d_k = torch.full((cap * ksz,), 0xFF, dtype=torch.uint8, device="cuda"); d_d = torch.full((cap * 32,), 0xFF, dtype=torch.uint8, device="cuda")
        d_n = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        e.copy_result(frame, d_k.data_ptr(), d_d.data_ptr(), d_n.data_ptr())
        e.sync()
        src_k = np.empty(cap * ksz, np.uint8); src_d = np.empty(cap * 32, np.uint8); src_n = np.empty(1, np.int32)
        for dst, ptr in ((src_k, k_ptr), (src_d, d_ptr), (src_n, n_ptr)):       # the HIP runtime the library is linked against, through its handle
            assert capi.lib().hipMemcpy(C.c_void_p(dst.ctypes.data), C.c_void_p(ptr), C.c_size_t(dst.nbytes), C.c_int(2)) == 0    # device to host
        assert 0 < src_n[0] < cap and d_n.cpu().numpy()[0] == src_n[0]
        assert np.array_equal(d_k.cpu().numpy(), src_k) and np.array_equal(d_d.cpu().numpy(), src_d)
    e.close()
