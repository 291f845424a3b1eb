"""tests/ba_resident_scene.py checked on the CPU: the windows it builds are what it says (exact counts, every observation a keypoint of its
camera's keyframe, kp = 0 and n - 1 and the first and last octave in use, unused / twice-seen / fixed-only points), the host gather is the
three casts, the restated pose_f32.h sequences agree with float64 algebra to float precision, and the prepare restatement does what
MapPoint::UpdateNormalAndDepth does on hand-made results -- including a scene where the order of a point's edges changes its normal's bits."""
import numpy as np

import ba_resident_scene as brs

F32 = np.float32


def test_windows_are_as_described():
    for (P, L, E, nf, kw) in ((3, 40, 1, 1, {}), (4, 63, 200, 2, dict(unused=3)), (5, 64, 257, 2, dict(twice=True, fixed_only=4)), (2, 1, 1, 1, {}),
                              (6, 257, 300, 3, dict(unused=5, outliers=0.1)), (3, 30, 60, 1, dict(behind=3))):
        sc = brs.make_window(7, P, L, E, nf, **kw)
        o = sc["obs"]
        assert len(o) == E and len(sc["records"]) == L and len(sc["kfs"]) == P and sc["fixed"].sum() == nf
        assert o["pose"].min() >= 0 and o["pose"].max() < P and o["point"].min() >= 0 and o["point"].max() < L
        for e in range(E):
            assert 0 <= o["kp"][e] < len(sc["kfs"][o["pose"][e]]["kps"])
        for p in range(P):           # a keypoint is the observation of at most one edge
            mine = o["kp"][o["pose"] == p]
            assert len(np.unique(mine)) == len(mine)
        cnt = np.bincount(o["point"], minlength=L)
        assert (cnt[L - kw.get("unused", 0):] == 0).all()
        assert ((sc["ref_edge"] == -1) == (cnt == 0)).all() and (o["point"][sc["ref_edge"][cnt > 0]] == np.flatnonzero(cnt > 0)).all()
        if kw.get("twice"):
            assert o["pose"][0] == o["pose"][-1] and o["point"][0] == o["point"][-1] and o["kp"][0] != o["kp"][-1]
        for l in range(kw.get("fixed_only", 0)):
            assert sc["fixed"][o["pose"][o["point"] == l]].all()
        if E >= L - kw.get("unused", 0):
            assert (cnt[:L - kw.get("unused", 0)] >= 1).all()
        mine0 = o["kp"][o["pose"] == 0]
        if len(mine0) >= 2:
            n0 = len(sc["kfs"][0]["kps"])
            assert n0 == len(mine0) and 0 in mine0 and n0 - 1 in mine0
            oct0 = sc["kfs"][0]["kps"]["octave"][mine0]
            assert 0 in oct0 and len(sc["kfs"][0]["scale_factors"]) - 1 in oct0
    n_obs = np.array([1, 2, 7, 0, 3] * 4)
    sc = brs.make_window(7, 8, 20, int(n_obs.sum()), 3, n_obs=n_obs)
    assert np.array_equal(np.bincount(sc["obs"]["point"], minlength=20), n_obs)
    sc = brs.make_window(7, 6, 40, 120, 2)
    assert len(sc["kfs"][2]["scale_factors"]) == 5 and len(sc["kfs"][0]["scale_factors"]) == 8
    assert sc["kfs"][2]["scale_factors"][1] == F32(1.1) and sc["kfs"][0]["scale_factors"][1] == F32(1.2)


def test_host_gather_is_the_three_casts():
    sc = brs.make_window(11, 4, 50, 150, 2)
    w = brs.host_window(sc)
    e, o = w["edges"], sc["obs"]
    assert np.array_equal(e["pose"], o["pose"]) and np.array_equal(e["point"], o["point"])
    for k in (0, 17, 149):
        kf = sc["kfs"][o["pose"][k]]; kp = kf["kps"][o["kp"][k]]
        assert e["u"][k] == float(kp["x"]) and e["v"][k] == float(kp["y"]) and F32(e["u"][k]) == kp["x"]
        assert e["inv_sigma2"][k] == float(kf["inv_level_sigma2"][kp["octave"]])
    assert w["points"].dtype == np.float64 and np.array_equal(w["points"].astype(F32), sc["records"]["pos"])
    assert len(set(e["inv_sigma2"])) > 8      # both level tables are in use
    s = brs.descending_slots(7, 40)
    assert s[0] == 39 and (np.diff(s) < -1).all() and len(set(np.diff(s))) == 2


def test_restated_pose_sequences_agree_with_float64_algebra():
    rng = np.random.default_rng(5)
    q = rng.normal(size=(200, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.uniform(-5, 5, (200, 3))
    ow = brs.se3_inverse_t(q.astype(F32), t.astype(F32))
    assert ow.dtype == F32
    ref = np.stack([-brs._R(q[i]).T @ t[i] for i in range(200)])
    assert np.abs(ow - ref).max() < 2e-5
    # the free camera's constructor normalisation: a quaternion 1e-4 off unit norm gives the centre of the normalised one
    poses = np.column_stack([t, q * 1.0001])
    c = brs.camera_centres(poses, poses, np.zeros(200, np.uint8))
    assert np.abs(c - ref).max() < 2e-5
    held = brs.camera_centres(poses, poses[::-1], np.ones(200, np.uint8))        # fixed: the input pose, poses_out is not read
    assert np.isfinite(held).all() and np.abs(held - ref).max() < 2e-3
    given = rng.normal(size=(200, 3)).astype(F32)
    fx = (np.arange(200) % 2).astype(np.uint8)
    mix = brs.camera_centres(poses, poses, fx, given)
    assert np.array_equal(mix[fx == 1], given[fx == 1]) and np.array_equal(mix[fx == 0], c[fx == 0])


def _fake_result(sc, chi2=1.0):
    return dict(poses=sc["poses"].copy(), points=sc["records"]["pos"].astype(np.float64), edge_chi2=np.full(sc["E"], chi2), depth_positive=np.ones(sc["E"], np.uint8))


def test_prepare_restatement():
    sc = brs.make_window(3, 5, 40, 160, 2, unused=4)
    res = _fake_result(sc)
    o = sc["obs"]
    res["edge_chi2"][np.flatnonzero(o["point"] == 0)[0]] = 5.992        # above the bound: dirty
    res["edge_chi2"][np.flatnonzero(o["point"] == 1)[0]] = 5.991        # at the bound: clean (a strict comparison)
    res["depth_positive"][np.flatnonzero(o["point"] == 2)[-1]] = 0
    geom, dirty, ow, state = brs.prepare_ref(sc, res)
    assert dirty[0] == 1 and dirty[1] == 0 and dirty[2] == 1 and dirty.sum() == 2
    assert (state[-4:] == 2).all() and (state[3:-4] == 0).all() and (geom[state != 0] == 0).all()
    ok = state == 0
    assert np.array_equal(geom[ok, :3], sc["records"]["pos"][ok])
    nrm = np.linalg.norm(geom[ok, 3:6].astype(np.float64), axis=1)
    assert (nrm <= 1 + 1e-6).all() and (nrm > 0.9).all()               # a mean of unit vectors that point the same way
    centres64 = np.stack([-brs._R(sc["poses"][p, 3:] / np.linalg.norm(sc["poses"][p, 3:])).T @ sc["poses"][p, :3] for p in range(sc["P"])])
    for l in np.flatnonzero(ok)[:10]:
        r = o[sc["ref_edge"][l]]
        kf = sc["kfs"][r["pose"]]
        dist = np.linalg.norm(sc["records"]["pos"][l].astype(np.float64) - centres64[r["pose"]])
        assert abs(geom[l, 7] - dist * kf["scale_factors"][kf["kps"]["octave"][r["kp"]]]) < 1e-4 * dist
        assert geom[l, 6] == F32(geom[l, 7] / kf["scale_factors"][-1])
    no_ref = brs.prepare_ref(sc, res, with_ref=False)[0]
    assert np.array_equal(no_ref[:, :6], geom[:, :6]) and (no_ref[:, 6:] == 0).all()
    rec = brs.committed_records(sc["records"], geom, state)
    assert rec[~ok].tobytes() == sc["records"][~ok].tobytes()
    for f in ("desc", "n_obs", "bad"):
        assert np.array_equal(rec[f], sc["records"][f])
    assert np.array_equal(rec["normal"][ok], geom[ok, 3:6]) and np.array_equal(rec["max_dist"][ok], geom[ok, 7])


def permuted(sc, rng):
    """the same window with its edge list in another order (ref_edge follows)"""
    perm = rng.permutation(sc["E"])
    inv = np.argsort(perm)
    ref = np.where(sc["ref_edge"] >= 0, inv[np.maximum(sc["ref_edge"], 0)], -1).astype(np.int32)
    return dict(sc, obs=sc["obs"][perm].copy(), ref_edge=ref), perm


def test_edge_order_changes_a_normals_bits():
    """float addition does not associate: with seven observers the order of the sum shows in the last bit of some normal"""
    sc = brs.make_window(21, 8, 30, 210, 2)
    assert np.bincount(sc["obs"]["point"]).max() >= 7
    res = _fake_result(sc)
    g0 = brs.prepare_ref(sc, res)[0]
    sp, perm = permuted(sc, np.random.default_rng(1))
    rp = dict(res, edge_chi2=res["edge_chi2"][perm], depth_positive=res["depth_positive"][perm])
    g1 = brs.prepare_ref(sp, rp)[0]
    assert np.array_equal(g0[:, :3], g1[:, :3]) and np.array_equal(g0[:, 6:], g1[:, 6:])
    assert (g0[:, 3:6].view(np.uint32) != g1[:, 3:6].view(np.uint32)).any()
    assert np.abs(g0 - g1).max() < 1e-6
