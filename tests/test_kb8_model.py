"""The KannalaBrandt8 restatement of tests/kb8_scene.py pinned against definitions that do not share its code -- its own inverse, central
differences, the pinhole limit -- and the host build of dvm_slam_amd/csrc/camera_model.h pinned against the restatement; then what the
scenes of tests/test_gpu_kb8.py hold: how many draws the chi2 margin discards, how many points the margin rule drops, and the pose
tolerance measured from one float32 ulp of theta.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kb8_scene as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rays(n, theta_max_deg, seed, theta_min_deg=0.0):
    rng = np.random.default_rng(seed)
    th = np.deg2rad(rng.uniform(theta_min_deg, theta_max_deg, n)); psi = rng.uniform(-np.pi, np.pi, n); d = rng.uniform(0.5, 30.0, n)
    return np.column_stack([d * np.sin(th) * np.cos(psi), d * np.sin(th) * np.sin(psi), d * np.cos(th)])


@pytest.mark.parametrize("model", list(ks.MODELS))
def test_unproject_inverts_project(model):
    """unproject(project(X)) is parallel to X for theta up to 85 deg, within the Newton precision the reference states: 1e-6."""
    p = ks.MODELS[model]
    X = _rays(4000, 85.0, 3)
    ray = ks.unproject(p, ks.project_f32(p, X)).astype(np.float64)
    cosang = (ray * X).sum(axis=1) / np.linalg.norm(ray, axis=1) / np.linalg.norm(X, axis=1)
    ang = np.arctan2(np.linalg.norm(np.cross(ray, X), axis=1), (ray * X).sum(axis=1))
    print("largest angle between unproject(project(X)) and X:", ang.max())
    assert cosang.min() > 0 and ang.max() < 1e-6


@pytest.mark.parametrize("model", list(ks.MODELS))
def test_project_jac_against_central_differences(model):
    """projectJac against central differences of the projection taken with the double atan2 (differences of the float-theta form are
    noise: it moves in steps of 3e-5 px).  Step h = 1e-6 |X|: truncation ~h^2, cancellation ~1e-16 / 1e-6 = 1e-10 relative."""
    p = ks.MODELS[model]
    X = _rays(3000, 85.0, 4, theta_min_deg=0.5)
    J = ks.project_jac(p, X)
    num = np.zeros_like(J)
    h = 1e-6 * np.linalg.norm(X, axis=1)
    for k in range(3):
        d = np.zeros_like(X); d[:, k] = h
        num[:, :, k] = (ks.project_exact(p, X + d) - ks.project_exact(p, X - d)) / (2 * h)[:, None]
    scale = np.abs(J).max(axis=(1, 2))
    err = np.abs(J - num).max(axis=(1, 2)) / scale
    print("largest relative difference:", err.max())
    assert err.max() < 1e-6
    # on the optical axis the reference's expressions are 0 / 0
    assert np.isnan(ks.project_jac(p, np.array([[0.0, 0.0, 2.0]]))).any()


def test_small_angle_limit_is_pinhole():
    """k = 0: u = fx theta x / rho + cx against the pinhole fx tan(theta) x / rho + cx: they differ by fx (tan(theta) - theta) <= fx theta^3 / 3 (1 + theta^2)."""
    p = np.array([500.0, 480.0, 320.0, 240.0, 0, 0, 0, 0], np.float32)
    X = _rays(2000, np.rad2deg(1e-3), 5)
    th = np.arctan2(np.hypot(X[:, 0], X[:, 1]), X[:, 2])
    pin = np.stack([500.0 * X[:, 0] / X[:, 2] + 320.0, 480.0 * X[:, 1] / X[:, 2] + 240.0], axis=1)
    d = np.abs(ks.project_exact(p, X) - pin).max(axis=1)
    assert np.all(d <= 500.0 * th ** 3 / 3 * (1 + th ** 2) + 1e-12)
    # the float theta and psi of project(Vector3d): x^2 + y^2, z, the square root and atan2f round theta by 3.5 half-ulps (2.1e-7 relative);
    # x, y and atan2f round psi by 6e-8 + 1.2e-7 rad (ulp of pi); both act on r f = 1e-3 x 500 px
    assert np.abs(ks.project_f64(p, X) - pin).max() < 500.0 * 1e-3 * (2.1e-7 + 1.8e-7) + 500.0 * 1e-9 / 3 + 1e-9
    assert np.abs(ks.project_f32(p, X).astype(np.float64) - pin).max() < 2e-4                            # float pixels near 320: ulp 3e-5


_SRC = r'''
#include "camera_model.h"
extern "C" void eval(const float* p, const double* X, int n, float* uvf, double* uvd, double* J, float* ray) {
  for (int i = 0; i < n; i++) {
    dvm_cam::kb8_project(p, (float)X[3 * i], (float)X[3 * i + 1], (float)X[3 * i + 2], uvf[2 * i], uvf[2 * i + 1]);
    dvm_cam::kb8_project(p, X[3 * i], X[3 * i + 1], X[3 * i + 2], uvd[2 * i], uvd[2 * i + 1]);
    dvm_cam::kb8_project_jac(p, X[3 * i], X[3 * i + 1], X[3 * i + 2], J + 6 * i);
    dvm_cam::kb8_unproject(p, uvf[2 * i], uvf[2 * i + 1], ray + 3 * i);
  }
}
extern "C" void pinhole(const float* p, const float* X, int n, float* uv) {
  for (int i = 0; i < n; i++) dvm_cam::project(0, p, X[3 * i], X[3 * i + 1], X[3 * i + 2], uv[2 * i], uv[2 * i + 1]);
}
'''


@pytest.fixture(scope="module")
def host_build():
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.cpp"), "w").write(_SRC)
        so = os.path.join(td, "libt.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "dvm_slam_amd", "csrc"), os.path.join(td, "t.cpp"), "-o", so])
        yield C.CDLL(so)


@pytest.mark.parametrize("model", list(ks.MODELS))
def test_host_build_of_camera_model_h(host_build, model):
    """dvm_slam_amd/csrc/camera_model.h compiled for the host against the restatement.  The header takes cos(psi), sin(psi) as x / rho,
    y / rho where the restatement takes psi from atan2f as the reference does: in the double projection that is half a float32 ulp of
    psi (<= 1.2e-7 rad) times r f (r <= 1.6 up to 85 deg), and the two atan2f may differ in the last bit of theta (1.2e-7 f'(theta) f)."""
    p = ks.MODELS[model]
    X = np.ascontiguousarray(_rays(5000, 85.0, 6, theta_min_deg=0.5))
    n = len(X)
    uvf = np.zeros((n, 2), np.float32); uvd = np.zeros((n, 2)); J = np.zeros((n, 6)); ray = np.zeros((n, 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    host_build.eval(vp(p), vp(X), C.c_int(n), vp(uvf), vp(uvd), vp(J), vp(ray))
    f = float(max(p[0], p[1]))
    d64 = np.abs(uvd - ks.project_f64(p, X)).max()
    d32 = np.abs(uvf.astype(np.float64) - ks.project_f32(p, X).astype(np.float64)).max()
    print("double projection: %.3g px, float projection: %.3g px" % (d64, d32))
    assert d64 < f * (1.6 * 1.2e-7 + 1.5 * 1.2e-7) + 1e-9
    assert d32 < 12 * 6.1e-5                # a dozen float32 roundings at up to 1 000 px (ulp 6.1e-5)
    Jr = ks.project_jac(p, X).reshape(n, 6)
    assert (np.abs(J - Jr).max(axis=1) / np.abs(Jr).max(axis=1)).max() < 1e-12
    rr = ks.unproject(p, uvf)
    assert np.abs(ray - rr).max() <= 4e-6 * np.abs(rr).max()       # op for op the same but tanf against numpy's tan: a few float32 ulps
    # the optical axis: the projection is the principal point, the Jacobian NaN as in the reference
    Z = np.array([[0.0, 0.0, 3.0]])
    host_build.eval(vp(p), vp(Z), C.c_int(1), vp(uvf), vp(uvd), vp(J), vp(ray))
    assert uvf[0, 0] == p[2] and uvf[0, 1] == p[3] and uvd[0, 0] == float(p[2]) and uvd[0, 1] == float(p[3]) and np.isnan(J[0]).any()


def test_host_build_pinhole_is_the_inline_formula(host_build):
    p = np.array([520.0, 390.0, 300.0, 250.0, 0, 0, 0, 0], np.float32)
    X = np.ascontiguousarray(_rays(1000, 60.0, 7).astype(np.float32))
    uv = np.zeros((len(X), 2), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    host_build.pinhole(vp(p), vp(X), C.c_int(len(X)), vp(uv))
    assert np.array_equal(uv[:, 0], p[0] * X[:, 0] / X[:, 2] + p[2]) and np.array_equal(uv[:, 1], p[1] * X[:, 1] / X[:, 2] + p[3])


def test_pose_scenes_margin_and_measured_tolerance():
    """Every scene of the GPU test: points reach 80 deg and stay off the axis, every classified chi2 is CHI2_MARGIN from 5.991, at most
    5 % of the draws were discarded for that, the planted outliers are what the restatement flags (the shift is far from the threshold
    under this camera too) -- and the tolerance: the restatement run again with every theta one float32 ulp off."""
    draws = discarded = 0
    D = 0.0
    for model, N in ks.pose_cases():
        sc, (T, outl, nin, info, off), nd = ks.pose_scene(model, N)
        draws += nd + 1; discarded += nd
        assert off and info["min_band"] >= ks.CHI2_MARGIN
        Xc = sc["Xw"] @ ks.quat_to_R(sc["pose_gt"][3:]).T + sc["pose_gt"][:3]
        th = np.arctan2(np.hypot(Xc[:, 0], Xc[:, 1]), Xc[:, 2])
        assert th.max() > np.deg2rad(79.9) and th.max() <= ks.THETA_MAX + 1e-9
        if N >= 64:
            # every planted outlier is flagged, and little else (0.7 px of noise passes 5.991 on 0.2 % of the finest-level edges)
            assert np.all(outl[sc["bad"]] == 1) and (outl[~sc["bad"]] == 1).sum() <= 0.01 * N + 1, (model, N)
            assert np.abs(T - sc["pose_gt"]).max() < 0.02
        print(f"{model} N={N}: seed {sc['seed']}, {nin} inliers")
    D = ks.theta_ulp_pose_diff()
    print("theta-ulp pose difference, largest:", D, "discarded draws:", discarded, "of", draws)
    assert discarded <= ks.DROP_MAX * draws
    # The GPU tolerance is 10 x this measurement.  THETA_ULP_POSE_DIFF (9.58e-6, docs/NOTEBOOK.md) is what it came to with one libm; one
    # scene whose last round can stop at either of two iterations sets it, so another atan2f may move it.  Asserted: a sane range --
    # above the 2e-8 that the best-conditioned scenes show, and small enough that 10 x it still tells a wrong Jacobian (1e-3 and more) apart.
    assert 2e-8 < D < 1e-4


def test_search_scenes_margin_rule():
    """The margin rule drops at most 5 % of a scene's points (none of a scene of 17 or fewer), and the scenes hold what they are for:
    visible points beyond 60 deg, points behind the camera, points outside the bounds, failed distance and viewing-angle tests, matches."""
    for model, seed, n_pts, n_kp, form in ks.search_cases():
        sc = ks.search_scene(model, seed, n_pts, n_kp, form == "fuse_sim3")
        r = ks.project_search_ref(sc, form, ks.SEARCH_TH[form])
        assert r["drop"].sum() <= ks.DROP_MAX * n_pts, (model, n_pts, n_kp, form)
        assert ((r["level"] >= 0) & ~r["drop"]).any(), (model, n_pts, n_kp, form)      # even the one-point scene has something to compare
        if n_pts == ks.PT_COUNTS[-1] and n_kp == ks.KP_COUNTS[-1]:
            Xc = sc["pos"].astype(np.float64) @ ks.quat_to_R(sc["q"].astype(np.float64)).T + sc["t"]
            th = np.arctan2(np.hypot(Xc[:, 0], Xc[:, 1]), Xc[:, 2])
            vis = r["level"] >= 0
            assert (vis & (th > np.deg2rad(60))).sum() > 20 and (Xc[:, 2] < 0).sum() > 50 and (~vis & (Xc[:, 2] > 0)).sum() > 100
            assert ((r["best_idx"] >= 0) & (r["best_dist"] <= 50)).sum() > 200
    for model in ks.MODELS:
        sc = ks.search_scene(model, 0, ks.PT_COUNTS[-1], ks.KP_COUNTS[-1])
        for n_pts in ks.PT_COUNTS:
            fr = ks.frustum_ref(ks.search_scene(model, 0, n_pts, ks.KP_COUNTS[-1]))
            assert ((fr["in_view"] == 1) & ~fr["drop"]).any(), (model, n_pts)
        f = ks.frustum_ref(sc)
        assert f["drop"].sum() <= ks.DROP_MAX * len(f["drop"]) and 300 < f["in_view"].sum() < 700
        fs = ks.frames_scene(model, 0)
        nm, mp, nq, frag = ks.frames_ref(fs, ks.FRAMES_TH)
        assert fs["n_dropped"] <= ks.DROP_MAX * len(fs["mp_l"]) and not frag.any() and nm > 150 and nq > 400


def test_entries_refuse_bad_models_before_looking_for_a_device(capi):
    """A NULL model, a model outside {0, 1} and a zero focal length are DVM_ERR_INVALID with or without a GPU; a good model without a GPU
    is DVM_ERR_NO_DEVICE, as for the pinhole siblings."""
    L = C.CDLL(capi.LIB_PATH)
    i32, f32, vp = C.c_int32, C.c_float, C.c_void_p
    z = np.zeros(256, np.float64)
    n = np.array([3], np.int32)
    ptr = lambda a: vp(a.ctypes.data)
    bad = [None, capi.CameraModel.make(2, ks.ROBOMASTER), capi.CameraModel.make(1, np.r_[ks.ROBOMASTER[:1], 0.0, ks.ROBOMASTER[2:]]),
           capi.CameraModel.make(0, np.r_[0.0, ks.ROBOMASTER[1:]])]
    good = [capi.CameraModel.robomaster(), capi.CameraModel.pinhole(500.0, 500.0, 320.0, 240.0)]
    assert C.sizeof(capi.CameraModel) == 36

    def calls(m):
        ref = None if m is None else C.byref(m)
        return [L.dvm_pose_optimize_cam(i32(0), ptr(z), ptr(z), ptr(z), ptr(z), ptr(n), i32(3), i32(1), ref, ptr(z), ptr(z), ptr(z)),
                L.dvm_is_in_frustum_cam(ptr(z), ref, ptr(z), ptr(z), ptr(z), ptr(z), i32(1), f32(0.5), ptr(z), i32(0), vp(0))]
    for m in bad:
        assert calls(m) == [-1, -1]
    if capi.device_count() == 0:
        for m in good:
            assert calls(m) == [-5, -5]
    assert np.all(z == 0)
