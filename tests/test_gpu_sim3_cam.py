"""GPU tests of the two Sim3 kernels on a camera model per keyframe (tests/sim3_cam_scene.py is the reference; tests/test_sim3_cam_scene.py
pins it on the CPU): dvm_sim3_hypotheses_cam (k_sim3_hypotheses<M1, M2>) and dvm_optimize_sim3_cam (k_optimize_sim3<M1, M2>).

Model 0 on both sides is the pinhole entry bit for bit.  On fisheye cameras the hypotheses' T12 keeps the pinhole entry's bits (Horn reads
no camera) and the mask equals the float64 decision on every clear pair; OptimizeSim3 returns the restatement's mask and count and S
within sim3_cam_scene.S_BOUND, ten times what one float ulp of theta moves the restatement."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import sim3_cam_scene as cs  # noqa: E402
import sim3_scene as ss  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def _cam(capi, m):
    return cs.camera_model(capi, m)


def _hyp(capi, sc, models, tri, fix):
    return capi.sim3_hypotheses_cam(sc["P1c"], sc["P2c"], sc["max_err1"], sc["max_err2"], _cam(capi, models[0]), _cam(capi, models[1]), tri, fix)


# ---- 5. model 0 is the old entry
@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("n", cs.HYP_N)
def test_hypotheses_model0_is_the_pinhole_entry(capi, n, fix):
    sc, gt = ss.scene(2, n, 0.3, 1.0)
    tri = ss.triples(2, n, cs.HYP_H)
    T0, n0, m0 = capi.sim3_hypotheses(triples=tri, fix_scale=fix, **sc)
    T, nin, mask = _hyp(capi, sc, (cs.pinhole(sc["K1"]), cs.pinhole(sc["K2"])), tri, fix)
    assert np.array_equal(_bits(T), _bits(T0)) and np.array_equal(nin, n0) and np.array_equal(mask, m0)
    if n >= 63:
        assert n0.max() >= 0.3 * n


@pytest.mark.parametrize("name", ["n10", "n255", "n256", "n257", "n513", "survive9", "survive10", "survive11", "fix_scale_1.3"])
def test_optimize_model0_is_the_pinhole_entry(capi, name):
    (S0, P1, P2, o1, o2, w1, w2, Ka, Kb), fix, th2, spec = ss.opt_case(name)
    Sa, ia, na = capi.optimize_sim3(S0, fix, P1, P2, o1, o2, w1, w2, Ka, Kb, th2)
    Sb, ib, nb = capi.optimize_sim3_cam(S0, fix, P1, P2, o1, o2, w1, w2, _cam(capi, cs.pinhole(Ka)), _cam(capi, cs.pinhole(Kb)), th2)
    assert np.array_equal(_bits(Sa), _bits(Sb)) and np.array_equal(ia, ib) and na == nb
    assert na == (0 if spec["second_round"] == 0 else ia.sum())


# ---- 6. hypotheses on fisheye cameras
@pytest.mark.parametrize("n", cs.HYP_N)
@pytest.mark.parametrize("pair", list(cs.PAIRS))
def test_hypotheses_on_camera_models(capi, pair, n):
    sc, gt, tri, models = cs.hyp_case(pair, n)
    for fix in (False, True):
        T, nin, mask = _hyp(capi, sc, models, tri, fix)
        # Horn's closed form reads no camera: the pinhole entry's bits on the same points, whatever its cameras
        T0 = capi.sim3_hypotheses(sc["P1c"], sc["P2c"], sc["max_err1"], sc["max_err2"], ss.K1, ss.K2, tri, fix)[0]
        assert np.array_equal(_bits(T), _bits(T0))
        assert np.array_equal(nin, mask.sum(axis=1)) and set(np.unique(mask)) <= {0, 1}
        gap_ok = ss.deviations(T, sc, tri, fix)[3] > ss.GAP_MIN
        ref, clear = ss.decide(*cs.inliers_cam_f64(T, sc, models), sc)
        assert (~gap_ok).mean() <= ss.GAP_SHARE_MAX and (~clear).mean() <= ss.BAND_SHARE_MAX
        use = clear & gap_ok[:, None]
        wrong = (mask.astype(bool) != ref) & use
        print(f"{pair} N={n} fix={fix}: compared {use.mean():.3f} of the pairs, inliers {ref[use].mean():.3f}, differing {int(wrong.sum())}")
        assert not wrong.any()
        if n >= 63:
            # the on-axis, z = 0 and z < 0 points: finite under KannalaBrandt8, decided as the restatement decides them
            for i in (cs.AXIS, cs.Z0, cs.BEHIND):
                assert use[:, i].mean() > 0.8 and np.array_equal(mask[:, i].astype(bool)[use[:, i]], ref[:, i][use[:, i]])
    if n >= 63 and models[0][0] == cs.KB8 and models[1][0] == cs.KB8:
        assert mask[:, [cs.AXIS, cs.Z0, cs.BEHIND]].any()            # (fix_scale: the last of the two runs) such a point can be an inlier


def test_hypotheses_model_is_read_per_side(capi):
    """Either fisheye model replaced by the pinhole model of its fx, fy, cx, cy changes at least 5 % of the clear decisions: all four
    instantiations read the model of the side they are given."""
    for pair in cs.PAIRS:
        sc, gt, tri, models = cs.hyp_case(pair, 257)
        T, nin, mask = _hyp(capi, sc, models, tri, False)
        clear = ss.decide(*cs.inliers_cam_f64(T, sc, models), sc)[1]
        for k in (0, 1):
            if models[k][0] != cs.KB8:
                continue
            other = tuple(cs.as_pinhole(m) if j == k else m for j, m in enumerate(models))
            T2, nin2, mask2 = _hyp(capi, sc, other, tri, False)
            both = clear & ss.decide(*cs.inliers_cam_f64(T, sc, other), sc)[1]
            assert np.array_equal(_bits(T2), _bits(T)) and (mask != mask2)[both].mean() >= ss.SWAP_SHARE_MIN


@pytest.mark.parametrize("pair", list(cs.PAIRS))
def test_hypothesis_rows_are_independent(capi, pair):
    """N = 65 (one lane into the second ballot round): the launch again, the rows permuted and one row alone give the same rows."""
    sc, gt, tri, models = cs.hyp_case(pair, 65)
    T, nin, mask = _hyp(capi, sc, models, tri, False)
    T2, nin2, mask2 = _hyp(capi, sc, models, tri, False)
    assert np.array_equal(_bits(T), _bits(T2)) and np.array_equal(nin, nin2) and np.array_equal(mask, mask2)
    perm = np.random.default_rng(9).permutation(len(tri))
    Tp, ninp, maskp = _hyp(capi, sc, models, tri[perm], False)
    assert np.array_equal(_bits(Tp), _bits(T[perm])) and np.array_equal(ninp, nin[perm]) and np.array_equal(maskp, mask[perm])
    r = int(np.argmax(nin))
    T1, nin1, mask1 = _hyp(capi, sc, models, tri[r:r + 1], False)
    assert np.array_equal(_bits(T1[0]), _bits(T[r])) and nin1[0] == nin[r] and np.array_equal(mask1[0], mask[r])


# ---- 7. OptimizeSim3 on fisheye cameras
def _opt(capi, name, S0=None):
    (S, *rest), fix, th2, spec, models = cs.opt_case_cam(name)
    return capi.optimize_sim3_cam(S if S0 is None else S0, fix, *rest, _cam(capi, models[0]), _cam(capi, models[1]), th2)


@pytest.mark.parametrize("name", [n for n in cs.OPT_CASES_CAM if n != cs.UNSTABLE_CASE])
def test_optimize_on_camera_models(capi, name):
    (S0, *rest), fix, th2, spec, models = cs.opt_case_cam(name)
    Sr, ir, nr = cs.opt_reference(name)
    Sg, ig, ng = _opt(capi, name)
    print(f"{name}: count {ng} (restatement {nr}), mask differs at {int((ig != ir).sum())}, |S - S_restatement| {np.abs(Sg - Sr).max():.3e} "
          f"(bound {cs.S_BOUND:.3e})")
    assert ng == nr and np.array_equal(ig, ir)
    if spec["second_round"] == 0:
        assert ng == 0 and not ig.any() and np.array_equal(_bits(Sg), _bits(np.asarray(S0)))
        return
    assert ng >= 10 and ng == ig.sum()
    assert np.abs(Sg - Sr).max() <= cs.S_BOUND
    if spec["survivors"] is not None:
        assert ng == spec["survivors"]
    if fix:
        assert np.array_equal(_bits(Sg[7:8]), _bits(np.float64([1.3])))


def test_optimize_quaternion_sign(capi):
    """S0 given as q and as -q: the same similarity within 1e-12."""
    S0 = cs.opt_case_cam("n257")[0][0]
    Sa, ia, na = _opt(capi, "n257")
    Sb, ib, nb = _opt(capi, "n257", np.r_[-S0[:4], S0[4:]])
    assert na == nb and np.array_equal(ia, ib)
    assert np.abs(ss.quat_to_R(Sa[:4]) - ss.quat_to_R(Sb[:4])).max() < 1e-12 and np.abs(Sa[4:] - Sb[4:]).max() < 1e-12


def test_optimize_is_repeatable(capi):
    a, b = _opt(capi, "n513"), _opt(capi, "n513")
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("name", ["n257", "survive9"])
def test_optimize_guarded_buffers(capi, name):
    """Every buffer the entry writes lies between guard words (N = 257: one pair into the second stride of 256 threads): S12, the mask and the
    count come back as from the plain call, the guards on both sides as they were -- after the early return too."""
    (S0, *rest), fix, th2, spec, models = cs.opt_case_cam(name)
    L = capi.lib()
    vp, i32 = C.c_void_p, C.c_int32
    L.dvm_optimize_sim3_cam.restype = i32
    L.dvm_optimize_sim3_cam.argtypes = [i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, C.c_double, vp, vp]
    n, G = len(rest[0]), 64
    arrs = [np.ascontiguousarray(a, np.float64) for a in rest]
    Sbuf = np.full(8 + 2 * G, 7.5); Sbuf[G:G + 8] = S0
    inl = np.full(n + 2 * G, 0xAA, np.uint8)
    cnt = np.full(1 + 2 * G, -77, np.int32)
    m1, m2 = _cam(capi, models[0]), _cam(capi, models[1])
    capi.check(L.dvm_optimize_sim3_cam(0, Sbuf[G:].ctypes.data, int(fix), *[a.ctypes.data for a in arrs], n, C.addressof(m1), C.addressof(m2), th2,
                                       inl[G:].ctypes.data, cnt[G:].ctypes.data))
    Sg, ig, ng = _opt(capi, name)
    assert np.array_equal(_bits(Sbuf[G:G + 8]), _bits(Sg)) and np.array_equal(inl[G:G + n], ig) and cnt[G] == ng
    assert (Sbuf[:G] == 7.5).all() and (Sbuf[G + 8:] == 7.5).all()
    assert (inl[:G] == 0xAA).all() and (inl[G + n:] == 0xAA).all() and (cnt[:G] == -77).all() and (cnt[G + 1:] == -77).all()
