"""GPU tests of dvm_ba_set_problem_cam (bundle adjustment on a camera model; k_edge_eval<JAC, CAM>):

  1. KannalaBrandt8, both cameras, cases a-e of tests/ba_kb8_scene.py, against the numpy restatement ba_f64: iterations, trials per iteration
     and stop reason equal; poses and points within the measured tolerance -- 10 x what one float32 ulp of every edge's theta moves the
     restatement itself by (the residual takes theta from atan2f, whose last bit differs between libm and the device), 1e-6 at least;
     per-edge chi2 within 10 x that scene's CPU chi2 difference; the chi2 > 5.991 classification and depth_positive equal on every edge;
  2. the pinhole guard: model 0 is dvm_ba_set_problem with the same four doubles, bit for bit (case a: the sequential-order window form,
     case d: the tile solver);
  3. one handle, pinhole -> KannalaBrandt8 -> pinhole: each result is a fresh handle's, bit for bit;
  4. two rounds on one graph as the welding BA runs them (optimize(5), outliers inactive and no robust kernel, optimize(10));
  5. determinism; a bad model and a zero focal length are DVM_ERR_INVALID.
No edge or point is dropped from a comparison.  tests/test_ba_kb8_model.py pins the restatement and the scenes on the CPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import ba_kb8_scene as bs  # noqa: E402
import kb8_scene as ks  # noqa: E402

pytestmark = pytest.mark.gpu
DVM_ERR_INVALID = -1


@pytest.fixture(scope="module")
def tol():
    """(pose, point) bounds: 10 x the measurement of this machine's CPU (a few seconds of numpy, computed once), 1e-6 at least."""
    return bs.tolerances()


def _model(capi, name):
    return capi.CameraModel.make(1, ks.MODELS[name])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _solve(capi, sc, model=None, intrinsics=None, iterations=bs.ITERATIONS, handle=None):
    """One problem on a handle (a fresh one unless given): (stats, poses, points, chi2, depth_positive)."""
    ba = handle or capi.BundleAdjuster()
    try:
        if model is not None:
            ba.set_problem_cam(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], model, bs.HUBER)
        else:
            ba.set_problem(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], intrinsics, bs.HUBER)
        st = ba.optimize(iterations)
        T, X = ba.result()
        chi, dp = ba.edge_chi2()
    finally:
        if handle is None:
            ba.close()
    return st, T, X, chi, dp


def _same_bits(a, b):
    return (a[0]["iterations"] == b[0]["iterations"] and list(a[0]["trials"]) == list(b[0]["trials"]) and a[0]["stop_reason"] == b[0]["stop_reason"]
            and _bits(np.array(a[0]["chi2"])).tolist() == _bits(np.array(b[0]["chi2"])).tolist()
            and _bits(np.array(a[0]["lam"])).tolist() == _bits(np.array(b[0]["lam"])).tolist()
            and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2])) and np.array_equal(_bits(a[3]), _bits(b[3]))
            and np.array_equal(a[4], b[4]))


def _depth_positive(T, X, edges):
    return (bs._camera_frame_points(T, X, edges)[:, 2] > 0).astype(np.uint8)


# ---- 1. KannalaBrandt8 against the restatement
@pytest.mark.parametrize("model,case", bs.all_cases())
def test_kb8_ba_matches_restatement(capi, tol, model, case):
    sc, ref, seed = bs.ba_case(model, case)
    st, T, X, chi, dp = _solve(capi, sc, model=_model(capi, model))
    dT, dX, dC = float(np.abs(T - ref["poses"]).max()), float(np.abs(X - ref["points"]).max()), float(np.abs(chi - ref["chi2"]).max())
    print(f"{model} {case} seed {seed}: trials {list(st['trials'])} / {ref['trials']}, stop {st['stop_reason']} / {ref['stop']}, "
          f"|dpose| {dT:.3e} (tol {tol[0]:.3e}), |dpoint| {dX:.3e} (tol {tol[1]:.3e}), |dchi2| {dC:.3e} (tol {10 * ref['dchi2']:.3e})")
    assert st["iterations"] == len(ref["trials"]) and list(st["trials"]) == ref["trials"] and st["stop_reason"] == ref["stop"]
    assert dT <= tol[0] and dX <= tol[1]
    assert dC <= 10 * ref["dchi2"]
    assert np.array_equal(chi > bs.CHI2_MONO, ref["chi2"] > bs.CHI2_MONO)
    assert np.array_equal(dp, _depth_positive(ref["poses"], ref["points"], sc["edges"]))


# ---- 2. the pinhole guard
@pytest.mark.parametrize("case", ["a", "d"])
def test_pinhole_model_is_set_problem(capi, case):
    sc = bs.ba_scene("pinhole", case, 0)
    K32 = np.array(bs.PINHOLE_K, np.float32)
    a = _solve(capi, sc, model=capi.CameraModel.make(0, K32))
    b = _solve(capi, sc, intrinsics=[float(v) for v in K32])
    assert a[0]["iterations"] >= 3
    assert _same_bits(a, b)


# ---- 3. one handle, three problems
def test_one_handle_pinhole_kb8_pinhole(capi):
    pin, fish = bs.ba_scene("pinhole", "c", 0), bs.ba_case("tum", "d")[0]
    K32 = np.array(bs.PINHOLE_K, np.float32)
    pm, km = capi.CameraModel.make(0, K32), _model(capi, "tum")
    fresh_pin, fresh_kb8 = _solve(capi, pin, model=pm), _solve(capi, fish, model=km)
    h = capi.BundleAdjuster()
    try:
        first = _solve(capi, pin, model=pm, handle=h)
        second = _solve(capi, fish, model=km, handle=h)
        third = _solve(capi, pin, model=pm, handle=h)
        plain = _solve(capi, pin, intrinsics=[float(v) for v in K32], handle=h)      # and dvm_ba_set_problem itself after a fisheye problem
    finally:
        h.close()
    assert _same_bits(first, fresh_pin) and _same_bits(second, fresh_kb8) and _same_bits(third, fresh_pin) and _same_bits(plain, fresh_pin)
    # the fisheye problem was not solved as a pinhole one: its observations read through the pinhole formula are another problem
    as_pin = _solve(capi, fish, intrinsics=[float(v) for v in ks.MODELS["tum"][:4]])
    assert float(np.abs(as_pin[1] - fresh_kb8[1]).max()) > 1e-3


# ---- 4. two rounds on one graph
@pytest.mark.parametrize("model", bs.MODELS)
def test_two_rounds_on_one_graph(capi, tol, model):
    sc, tr, seed = bs.two_round_case(model, "d")
    ba = capi.BundleAdjuster()
    try:
        ba.set_problem_cam(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], _model(capi, model), bs.HUBER)
        st1 = ba.optimize(5)
        chi1, _ = ba.edge_chi2()
        flags = np.where(chi1 > bs.CHI2_MONO, 0, capi.BA_EDGE_ACTIVE).astype(np.uint8)     # outliers to level 1, no robust kernel anywhere
        ba.set_edge_flags(flags)
        st2 = ba.optimize(10)
        T, X = ba.result()
        chi2, dp = ba.edge_chi2()
    finally:
        ba.close()
    r1, r2 = tr["round1"], tr["round2"]
    dT, dX, dC = float(np.abs(T - r2[0]).max()), float(np.abs(X - r2[1]).max()), float(np.abs(chi2 - r2[4]).max())
    print(f"{model} d seed {seed}: round 1 {list(st1['trials'])} / {r1[2]}, round 2 {list(st2['trials'])} / {r2[2]} stop {st2['stop_reason']} / {r2[3]}, "
          f"|dpose| {dT:.3e} (tol {tol[0]:.3e}), |dpoint| {dX:.3e} (tol {tol[1]:.3e}), |dchi2| {dC:.3e} (tol {10 * tr['dchi2']:.3e})")
    assert list(st1["trials"]) == r1[2] and st1["stop_reason"] == r1[3]
    assert np.array_equal(flags & 1, tr["flags"])
    assert list(st2["trials"]) == r2[2] and st2["stop_reason"] == r2[3]
    assert dT <= tol[0] and dX <= tol[1]
    assert dC <= 10 * max(tr["dchi2"], tr["dchi2_1"])             # (a level-1 edge keeps its round-1 chi2)
    assert np.array_equal(chi2 > bs.CHI2_MONO, r2[4] > bs.CHI2_MONO)
    assert np.array_equal(dp, _depth_positive(r2[0], r2[1], sc["edges"]))


# ---- 5. determinism, bad models
def test_kb8_ba_is_deterministic(capi):
    sc = bs.ba_case("robomaster", "e")[0]
    m = _model(capi, "robomaster")
    assert _same_bits(_solve(capi, sc, model=m), _solve(capi, sc, model=m))


def test_bad_model_is_invalid(capi):
    sc = bs.ba_scene("robomaster", "a", 0)
    ba = capi.BundleAdjuster()
    try:
        for bad in (capi.CameraModel.make(7, ks.MODELS["robomaster"]), capi.CameraModel.make(1, [0.0] + list(ks.MODELS["robomaster"][1:])),
                    capi.CameraModel.make(0, [0.0, 380.0, 480.0, 270.0])):
            with pytest.raises(capi.DvmError) as ei:
                ba.set_problem_cam(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], bad, bs.HUBER)
            assert ei.value.code == DVM_ERR_INVALID
        with pytest.raises(capi.DvmError):      # nothing was set
            ba.optimize(1)
    finally:
        ba.close()
