"""The projection-search kernels with fx != fy and a camera, bounds and pyramid per keyframe (tests/camera_scene.py): k_project_search,
k_is_in_frustum, k_match_triangulation, k_triangulate_matches, the whole ORBmatcher functions over them, and the FuseTargets, NewPoints and
tracking chains.  Every case asserts the device equal to the oracle bit for bit, in the fields the existing test of that entry compares,
and equal to the plain float64 statements on every item outside the band, with the continuous outputs within four times the deviation
tests/test_camera_scene.py records for the oracle.  The scenes are pinned by that file on the CPU: a camera entry, a camera or bounds
taken from the wrong place change 30 % or more of their matches, so any such exchange in a kernel or in the host code that fills its
camera fails the first assertion of the case that runs it."""
import functools

import numpy as np
import pytest

import camera_scene as cs
import fuse_targets_scene as fts
import new_points_scene as nps
import tri_scene
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

MEASURED = {}           # name -> largest deviation of the device from float64 seen in this run


def _hold(name, dev):
    for k, v in (dev.items() if isinstance(dev, dict) else [("", dev)]):
        key = f"{name}.{k}" if k else name
        MEASURED[key] = max(MEASURED.get(key, 0.0), float(v))
        assert v <= 4 * cs.ORACLE_DEV[key], f"{key}: {v:.3e} above 4 x {cs.ORACLE_DEV[key]:.3e}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module's tests: the largest deviations of the device from float64 seen in this run (shown with pytest -s)."""
    yield
    for k in sorted(MEASURED):
        print(f"{k:28s} {MEASURED[k]:.3e}   bound {4 * cs.ORACLE_DEV[k]:.3e}")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ project_search
@pytest.mark.parametrize("th,gate,masks", cs.PROJECT_SEARCH_MODES)
@pytest.mark.parametrize("cam", ["A", "B"])
@pytest.mark.parametrize("seed", [0, 1])
def test_project_search(capi, seed, cam, th, gate, masks):
    sc = cs.project_search_scene(po, seed, cam)
    pts = sc["pts"]
    for v, kf in enumerate(sc["kf"]):
        skip, valid = cs.project_search_masks(sc, v, seed) if masks else (None, pts["valid"])
        gi = kf["inv_level_sigma2"] if gate else None
        bi_o, bd_o, pr_o = po.project_search(kf["kps"], kf["desc"], kf["bounds"], skip, kf["Tcw"], po.se3_inverse(kf["Tcw"])[4:], kf["K"], dict(pts, valid=valid),
                                             th, kf["scale_factors"], kf["log_scale_factor"], gi, 5.99)
        g = capi.FrameGrid(2048)
        g.build(kf["kps"], kf["desc"], tuple(float(x) for x in kf["bounds"]))
        cam_d = dict(Tcw=kf["Tcw"], Ow=capi.se3_inverse(kf["Tcw"])[4:], K=kf["K"], bounds=kf["bounds"], log_scale_factor=kf["log_scale_factor"])
        m, pr = capi.project_search(g, cam_d, pts, th, kf["scale_factors"], skip=skip, gate_inv_sigma2=gi, gate=5.99, valid=valid)
        g.close()
        assert np.array_equal(pr["level"], pr_o[:, 3].astype(np.int32))
        ok = pr["level"] >= 0
        assert ok.sum() > 400
        for f, col in (("u", 0), ("v", 1), ("radius", 2)):
            assert np.array_equal(_bits(pr[f][ok]), _bits(pr_o[ok, col])), f
        assert np.array_equal(m["best_idx"], bi_o) and np.array_equal(m["best_dist"], bd_o)
        r = cs.project_search_f64(kf, pts, th, gate, skip, valid)
        _hold("project_search", cs.check_project_search(m["best_idx"], m["best_dist"], pr["level"], pr["u"], pr["v"], pr["radius"], r, f"device, kf {v}",
                                                                second_dist=m["second_dist"]))


# ------------------------------------------------------------------------------------------------------------------------- frustum
@pytest.mark.parametrize("cam", ["A", "B"])
def test_is_in_frustum(capi, cam):
    F, pts = cs.frustum_case(cam)
    want = cs.run_frustum(po, F, pts)
    got = cs.run_frustum(capi, F, pts)
    assert want["in_view"].sum() > 400
    for f in ("in_view", "level", "proj_x", "proj_y", "proj_xr", "depth", "view_cos"):
        assert np.array_equal(got[f], want[f]), f
    _hold("frustum", cs.check_frustum(got, cs.frustum_f64(F, pts), "device"))


# ------------------------------------------------------------------------------------------------------- triangulation search
@pytest.mark.parametrize("coarse", [False, True], ids=["fine", "coarse"])
@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("seed", [0, 1, "epipole"])
def test_triangulation_search(capi, seed, order, coarse):
    k1, k2 = cs.triangulation_pair(po, seed, order)
    va, vb = capi.keyframe_view(dict(k1, mp=k1["mp"].copy())), capi.keyframe_view(dict(k2, mp=k2["mp"].copy()))
    geo_o = po.triangulation_geometry(k1["Tcw"], k2["Tcw"], k1["K"], k2["K"])
    geo_g = capi.triangulation_geometry(va, vb)
    for x, y in zip(geo_o, geo_g):
        assert np.array_equal(_bits(x), _bits(y))
    for ori in (True, False):
        n_o, p_o = po.search_for_triangulation(k1["kps"], k1["desc"], k1["mp"], k1["fv"], k2["kps"], k2["desc"], k2["mp"], k2["fv"], geo_o[3], geo_o[2],
                                               k2["scale_factors"], k2["level_sigma2"], coarse, ori)
        n_g, p_g = capi.search_for_triangulation(va, vb, coarse, ori)
        assert n_g == n_o and np.array_equal(p_g, p_o)
    if seed != "epipole":
        assert n_o > 150
    match, tie, clear, geo = cs.triangulation_search_f64(k1, k2, coarse)
    cs.check_pairs(p_g, len(k1["kps"]), match, tie, clear, "device")          # (the orientation-free run)
    _hold("triangulation", cs.check_geometry(geo_g[2], geo_g[3], geo))


# ------------------------------------------------------------------------------------------------------------ triangulate_matches
@pytest.mark.parametrize("far", [False, True], ids=["plain", "far_points"])
@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("n", [129, 700])
def test_triangulate_matches(capi, n, order, far):
    S, kw = cs.triangulate_case(n, order, far)
    args = (S["K1"], S["K2"], S["T1w"], S["T2w"], S["Ow1"], S["Ow2"], S["kps1"], S["kps2"], S["pairs"], S["sigma2_1"], S["sigma2_2"], S["sf1"], S["sf2"],
            S["ratio_factor"])
    Xo, so = po.triangulate_matches(*args, **kw)
    Xg, sg = capi.triangulate_matches(*args, **kw)
    assert np.array_equal(sg, so) and np.array_equal(_bits(Xg), _bits(Xo))
    X64, st64, margin = tri_scene.numpy_reference(S, **kw)
    clear = margin > cs.TRI_BAND
    assert np.array_equal(sg[clear], st64[clear])
    made = clear & (st64 == 0)
    assert made.sum() > n // 4
    _hold("triangulate.X", float(np.max(np.linalg.norm(Xg[made] - X64[made], axis=1) / np.linalg.norm(X64[made], axis=1))))


# ---------------------------------------------------------------------------------------------------------------- whole functions
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("name", cs.WHOLE_FUNCTIONS)
def test_whole_function(capi, name, seed):
    """fuse, fuse_sim3, search_by_projection_sim3, search_by_projection_reloc, search_by_projection_frames on A; search_by_sim3 on
    camera_scene.sim3_pair.  The reference is the oracle alone; the oracle called with a wrong camera must answer otherwise."""
    sc, wrong = cs.whole_function_scene(po, name, seed)
    n_o, r_o = cs.whole_function(po, name, sc, seed)
    n_g, r_g = cs.whole_function(capi, name, sc, seed)
    assert n_g == n_o and np.array_equal(r_g, r_o)
    assert n_o > 100
    n_w, r_w = cs.whole_function(po, name, wrong, seed)
    assert cs.changed_share(r_o, r_w, r_o >= 0) >= cs.SWAP_SHARE_MIN


# ---------------------------------------------------------------------------------------------------------------- the Fuse chain
@pytest.fixture(scope="module")
def ft_chain(capi):
    h = capi.FuseTargets()
    h.reserve(200, 5, 5 * 300 + 2000)
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def _ft_f64(n):
    sc = cs.fuse_targets(0, n)
    return cs.fuse_rows_f64(sc["targets"], sc["pts"], sc["skip"])


@pytest.mark.parametrize("n", [1, 17, 200])
def test_fuse_targets(ft_chain, n):
    sc = cs.fuse_targets(0, n)
    ft_chain.set(sc["targets"])
    for skip in (sc["skip"], None):
        bi, bd = ft_chain.run(sc["pts"], 3.0, skip)
        want_i, want_d = fts.oracle_rows(sc["targets"], sc["pts"], skip)
        assert np.array_equal(bi, want_i) and np.array_equal(bd, want_d)
    bi, bd = ft_chain.run(sc["pts"], 3.0, sc["skip"])
    cs.check_fuse_rows(bi, bd, *_ft_f64(n), what="device")
    if n == 200:
        assert np.all((bi >= 0).sum(axis=1)[[0, 2, 3, 4]] > 30) and np.all(bi[fts.EMPTY_TARGET] == -1)


@pytest.mark.parametrize("what", ["cameras", "bounds"])
def test_fuse_targets_two_targets_exchange(ft_chain, what):
    """Two targets exchange cameras (bounds): their rows change, by float64 and on the device; the rows of the others keep their bits."""
    sc = cs.fuse_targets(0, 200)
    a, b = cs.FT_EXCHANGE[what]
    ft_chain.set(sc["targets"])
    base_i, base_d = ft_chain.run(sc["pts"], 3.0, sc["skip"])
    wrong = cs.ft_wrong(sc["targets"], what)
    ft_chain.set(wrong)
    bi, bd = ft_chain.run(sc["pts"], 3.0, sc["skip"])
    want_i, want_d = fts.oracle_rows(wrong, sc["pts"], sc["skip"])
    assert np.array_equal(bi, want_i) and np.array_equal(bd, want_d)
    f_i, f_d, f_ties, f_clear = cs.fuse_rows_f64(wrong, sc["pts"], sc["skip"])
    cs.check_fuse_rows(bi, bd, f_i, f_d, f_ties, f_clear, what="device")
    b64 = _ft_f64(200)[0]
    for t in range(5):
        if t in (a, b):
            assert cs.changed_share(base_i[t], bi[t], base_i[t] >= 0) >= cs.SWAP_SHARE_MIN
            assert cs.changed_share(b64[t], f_i[t], b64[t] >= 0) >= cs.SWAP_SHARE_MIN
        else:
            assert bi[t].tobytes() == base_i[t].tobytes() and bd[t].tobytes() == base_d[t].tobytes()


# ----------------------------------------------------------------------------------------------------------- the NewPoints chain
@pytest.fixture(scope="module")
def np_chain(capi):
    h = capi.NewPoints()
    h.reserve(2048, 30, 30 * 1024)
    yield h
    h.close()


def _np_run(h, sc, **kw):
    return h.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"], **kw)


@pytest.mark.parametrize("check_ori", [False, True], ids=["plain", "check_ori"])
@pytest.mark.parametrize("n", [5, 30])
def test_new_points(np_chain, n, check_ori):
    sc = cs.new_points(0, n)
    want = nps.oracle_chain(sc, check_ori=check_ori)
    got = _np_run(np_chain, sc, check_ori=check_ori)
    nps.assert_same(got, want)
    assert (got["status"] == 0).sum() >= 150 and (got["nb_status"] == 1).sum() >= 1
    if not check_ori:
        _hold("new_points.X", cs.check_new_points(got, sc, cs.new_points_f64(sc), "device"))


def _rows(res, j):
    s = slice(res["pair_off"][j], res["pair_off"][j + 1])
    return res["pairs"][s], res["status"][s], res["x3D"][s]


def test_new_points_two_neighbours_exchange_cameras(np_chain):
    """Neighbours 3 (on B) and 4 (on A) exchange cameras: their rows change, by float64 and on the device; the rows of the neighbours
    before them keep their bits (the later ones see another table of the current keyframe)."""
    sc = cs.new_points(0, 5)
    a, b = cs.NP_EXCHANGE
    base = _np_run(np_chain, sc)
    wrong = cs.np_wrong(sc, "cameras")
    got = _np_run(np_chain, wrong)
    nps.assert_same(got, nps.oracle_chain(wrong))
    f64, g64 = cs.new_points_f64(sc), cs.new_points_f64(wrong)
    cs.check_new_points(got, wrong, g64, "device")
    n1 = len(sc["cur"]["kps"])
    for j in range(5):
        if base["nb_status"][j] == 1:
            assert got["nb_status"][j] == 1
            continue
        if j in (a, b):
            m0 = np.full(n1, -1); m0[_rows(base, j)[0][:, 0]] = _rows(base, j)[0][:, 1]
            m1 = np.full(n1, -1); m1[_rows(got, j)[0][:, 0]] = _rows(got, j)[0][:, 1]
            assert cs.changed_share(m0, m1, m0 >= 0) >= cs.SWAP_SHARE_MIN
            assert cs.changed_share(f64[j]["match"], g64[j]["match"], f64[j]["match"] >= 0) >= cs.SWAP_SHARE_MIN
        elif j < min(a, b):
            for x, y in zip(_rows(base, j), _rows(got, j)):
                assert x.tobytes() == y.tobytes()


def test_new_points_two_neighbours_exchange_bounds(np_chain):
    """CreateNewMapPoints reads no keyframe's bounds (tests/test_camera_scene.py shows it on the float64 statement): with the bounds of two
    neighbours exchanged every row keeps its bits."""
    sc = cs.new_points(0, 5)
    base = _np_run(np_chain, sc)
    got = _np_run(np_chain, cs.np_wrong(sc, "bounds"))
    for k in base:
        assert base[k].tobytes() == got[k].tobytes(), k


# ------------------------------------------------------------------------------------------------------------------ the tracker
def test_tracker_on_camera_A(capi):
    """Tracker.track + track_local_map on frames rendered through CAM_A: the fused chain against the separate calls (bit for bit) and
    against the same composition over the oracle, as tests/test_gpu_track_local_map.py composes them; the oracle composition called with
    fx and fy exchanged assigns otherwise."""
    import pixel_scene as ps
    import test_gpu_track_local_map as tlm
    KA = np.array(cs.CAM_A, np.float32)
    frames, poses = ps.render(3, K=np.array(cs.CAM_A))
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(5)
    tabs = []
    for f in (0, 1, 2):                                           # the local map: the back-projected keypoints of three frames, frame 0's first
        n, k, d, _ = ext.extract(frames[f])
        R, t = poses[f]
        tabs.append(tlm._local_points(capi, k, d, ps.backproject(k, R, t, K=np.array(cs.CAM_A)) + rng.normal(0, 0.01, (n, 3)), -R.T @ t, scale, rng))
        if f == 0:
            k0, n0 = k.copy(), n
    pts = np.concatenate(tabs)
    trk = capi.Tracker(ext)
    trk.reserve_local_map(len(pts))
    first = trk.track(frames[1], tlm._tcw7f(ps.pose7(*poses[0])), KA, tlm.BOUNDS, scale, inv_s2, k0, np.arange(n0, dtype=np.int32), None, tlm._mps(capi, pts), th=15.0)
    assert first["tracked"]
    fused = tlm._run_both(capi, po, trk, first, pts, scale, inv_s2, 5.0, False, 0.0, K=KA)
    assert fused["nmatches"] > 100
    wrong = tlm._separate(po, first["kps_un"], first["desc"], first["mp"], pts, first["Tcw"], KA[[1, 0, 2, 3]], tlm.BOUNDS, scale, inv_s2, 5.0, False, 0.0)
    new = (fused["mp"] >= 0) & (fused["mp"] != first["mp"])
    assert new.sum() > 50 and cs.changed_share(fused["mp"], wrong["mp"], new) >= cs.SWAP_SHARE_MIN
    trk.close(); ext.close()
