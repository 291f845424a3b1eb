"""GPU tests of dvm_ba_optimize_windows_fast_cam / dvm_ba_pool_optimize_cam (k_ba_window_cluster<CAM>: the batched local-BA windows on a
camera model per window).  Scenes: tests/ba_kb8_window_scene.py -- robomaster and tum on the five shapes of tests/ba_kb8_scene.py, on
w30 (30 free cameras) and on w1 (one free camera).

  1. all 14 scenes in ONE call, robomaster and tum alternating, against the numpy restatement ba_f64: iterations, trials per iteration
     and stop reason equal; poses and points within 10 x what one float32 ulp of every edge's theta moves the restatement by over
     exactly these scenes (1e-6 at least); per-edge chi2 within 10 x the scene's own chi2 difference; the chi2 > 5.991 classification
     and depth_positive equal on every edge;
  2. the same windows against the tile solver (dvm_ba_set_problem_cam + dvm_ba_optimize: the same kb8_project, so the same theta bits,
     another summation order): the same trial sequence and stop reason, states within the larger of 1e-6 and 10 x the distance between
     the two forms on the pinhole twin of the scene (ba_optimize_windows(fast=True) against BundleAdjuster.set_problem: both as they
     were before this entry existed);
  3. the pinhole guard: model 0 windows equal dvm_ba_optimize_windows_fast on the same four doubles, bit for bit;
  4. a call of pinhole, robomaster and tum windows interleaved: every window has the bits of its solo call and of the reversed call;
  5. the bits depend neither on the cluster size G nor on the G = 1 repeat after a barrier time-out;
  6. the pool: four threads, four models, every result the bits of a solo call;
  7. the edges of the contract: 31 free cameras, a bad model, iterations = 0 and a window without edges in a mixed call, determinism;
  8. a fisheye window solved as a pinhole one is another problem.
No edge, point or scene is dropped from a comparison.  tests/test_ba_kb8_window_scene.py pins the scenes on the CPU."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import ba_kb8_scene as bs  # noqa: E402
import ba_kb8_window_scene as ws  # noqa: E402
import kb8_scene as ks  # noqa: E402

pytestmark = pytest.mark.gpu
DVM_ERR_INVALID, DVM_ERR_CAPACITY = -1, -3
K32 = np.array(bs.PINHOLE_K, np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _model(capi, name):
    return capi.CameraModel.make(0, K32) if name == "pinhole" else capi.CameraModel.make(1, ks.MODELS[name])


def _window(capi, sc, model=None, intrinsics=None, iterations=bs.ITERATIONS):
    w = dict(poses=sc["poses0"], fixed=sc["fixed"], points=sc["points0"], edges=sc["edges"], huber_delta=bs.HUBER, iterations=iterations)
    if model is not None:
        w["model"] = _model(capi, model)
    else:
        w["intrinsics"] = intrinsics
    return w


def _copy(g):
    return dict(poses=g["poses"].copy(), points=g["points"].copy(), edge_chi2=g["edge_chi2"].copy(), depth_positive=g["depth_positive"].copy(),
                stats=dict(g["stats"]))


def _run(capi, wins):
    return [_copy(g) for g in capi.ba_optimize_windows(wins, fast=True)]


def _same_bits(a, b):
    sa, sb = a["stats"], b["stats"]
    return (sa["iterations"] == sb["iterations"] and list(sa["trials"]) == list(sb["trials"]) and sa["stop_reason"] == sb["stop_reason"]
            and _bits(sa["chi2"]).tolist() == _bits(sb["chi2"]).tolist() and _bits(sa["lam"]).tolist() == _bits(sb["lam"]).tolist()
            and np.array_equal(_bits(a["poses"]), _bits(b["poses"])) and np.array_equal(_bits(a["points"]), _bits(b["points"]))
            and np.array_equal(_bits(a["edge_chi2"]), _bits(b["edge_chi2"])) and np.array_equal(a["depth_positive"], b["depth_positive"]))


def _depth_positive(T, X, edges):
    return (bs._camera_frame_points(T, X, edges)[:, 2] > 0).astype(np.uint8)


@pytest.fixture(scope="module")
def tol():
    """(pose, point) bounds: 10 x the measurement of this machine's CPU over the 14 scenes (computed once), 1e-6 at least."""
    return ws.tolerances()


@pytest.fixture(scope="module")
def fleet(capi):
    """The 14 admitted scenes, their references, and their windows solved in ONE dvm_ba_optimize_windows_fast_cam call."""
    cases = ws.window_cases()
    scenes = [ws.case(m, n) for m, n in cases]
    res = _run(capi, [_window(capi, sc, model=m) for (m, n), (sc, ref, seed) in zip(cases, scenes)])
    return cases, scenes, res


# ---- 1. against the restatement
def test_one_call_of_14_windows_matches_restatement(fleet, tol):
    cases, scenes, res = fleet
    assert len(cases) == 14 and {m for m, n in cases} == set(bs.MODELS) and [m for m, n in cases[:2]] == list(bs.MODELS)
    failures = []
    for (model, name), (sc, ref, seed), g in zip(cases, scenes, res):
        st = g["stats"]
        dT, dX = float(np.abs(g["poses"] - ref["poses"]).max()), float(np.abs(g["points"] - ref["points"]).max())
        dC = float(np.abs(g["edge_chi2"] - ref["chi2"]).max())
        print(f"{model} {name} seed {seed}: trials {list(st['trials'])} / {ref['trials']}, stop {st['stop_reason']} / {ref['stop']}, "
              f"|dpose| {dT:.3e} (tol {tol[0]:.3e}), |dpoint| {dX:.3e} (tol {tol[1]:.3e}), |dchi2| {dC:.3e} (tol {10 * ref['dchi2']:.3e})")
        ok = (st["iterations"] == len(ref["trials"]) and list(st["trials"]) == ref["trials"] and st["stop_reason"] == ref["stop"]
              and dT <= tol[0] and dX <= tol[1] and dC <= 10 * ref["dchi2"]
              and np.array_equal(g["edge_chi2"] > bs.CHI2_MONO, ref["chi2"] > bs.CHI2_MONO)
              and np.array_equal(g["depth_positive"], _depth_positive(ref["poses"], ref["points"], sc["edges"])))
        if not ok:
            failures.append((model, name))
    assert not failures, failures


# ---- 2. against the tile solver on the same device
def _tile(capi, sc, model=None, intrinsics=None):
    ba = capi.BundleAdjuster()
    try:
        if model is not None:
            ba.set_problem_cam(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], _model(capi, model), bs.HUBER)
        else:
            ba.set_problem(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], intrinsics, bs.HUBER)
        st = ba.optimize(bs.ITERATIONS)
        T, X = ba.result()
    finally:
        ba.close()
    return st, T, X


def test_windows_match_the_tile_solver(capi, fleet):
    cases, scenes, res = fleet
    failures = []
    for (model, name), (sc, ref, seed), g in zip(cases, scenes, res):
        twin = ws.pinhole_twin(name, seed)
        pw = _run(capi, [_window(capi, twin, intrinsics=bs.PINHOLE_K)])[0]
        pst, pT, pX = _tile(capi, twin, intrinsics=bs.PINHOLE_K)
        yT, yX = float(np.abs(pw["poses"] - pT).max()), float(np.abs(pw["points"] - pX).max())
        st, T, X = _tile(capi, sc, model=model)
        dT, dX = float(np.abs(g["poses"] - T).max()), float(np.abs(g["points"] - X).max())
        tT, tX = max(1e-6, 10 * yT), max(1e-6, 10 * yX)
        print(f"{model} {name} seed {seed}: trials {list(g['stats']['trials'])} / {list(st['trials'])}, pinhole twin's two forms differ by {yT:.3e} / {yX:.3e}; "
              f"fisheye |dpose| {dT:.3e} (tol {tT:.3e}), |dpoint| {dX:.3e} (tol {tX:.3e})")
        ok = (list(g["stats"]["trials"]) == list(st["trials"]) and g["stats"]["stop_reason"] == st["stop_reason"]
              and g["stats"]["iterations"] == st["iterations"] and dT <= tT and dX <= tX)
        if not ok:
            failures.append((model, name))
    assert not failures, failures


# ---- 3. the pinhole guard
def test_model_0_windows_are_the_pinhole_call(capi):
    twins = [ws.pinhole_twin(n, 0) for n in ("a", "d", "w30")]
    a = _run(capi, [_window(capi, sc, model="pinhole") for sc in twins])
    b = _run(capi, [_window(capi, sc, intrinsics=[float(v) for v in K32]) for sc in twins])
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["stats"]["iterations"] >= 3, k
        assert _same_bits(x, y), k


# ---- 4. a mixed call
def test_mixed_call_has_the_bits_of_solo_calls(capi):
    mix = [("pinhole", "a"), ("robomaster", "a"), ("tum", "d"), ("pinhole", "d"), ("robomaster", "w1"), ("tum", "a"), ("pinhole", "w1"), ("robomaster", "d")]
    wins = [_window(capi, ws.pinhole_twin(n, 0) if m == "pinhole" else ws.case(m, n)[0], model=m) for m, n in mix]
    both = _run(capi, wins)
    rev = _run(capi, wins[::-1])[::-1]
    for k, w in enumerate(wins):
        solo = _run(capi, [w])[0]
        assert both[k]["stats"]["iterations"] >= 3, mix[k]
        assert _same_bits(both[k], solo) and _same_bits(both[k], rev[k]), mix[k]


# ---- 5. independence of G and of the time-out repeat
def test_bits_do_not_depend_on_the_cluster_size_or_the_repeat(capi, monkeypatch):
    wins = [_window(capi, ws.case("robomaster", n)[0], model="robomaster") for n in ("a", "d", "e", "w30")]
    ref = _run(capi, wins)
    for G in (1, 2, 4, 8):
        monkeypatch.setenv("DVM_BA_CLUSTER", str(G))
        res = _run(capi, wins)
        for k, (a, b) in enumerate(zip(ref, res)):
            assert _same_bits(a, b), (G, k)
    monkeypatch.delenv("DVM_BA_CLUSTER")
    monkeypatch.setenv("DVM_BA_TEST_TIMEOUT", "1")
    res = _run(capi, wins)
    for k, (a, b) in enumerate(zip(ref, res)):
        assert _same_bits(a, b), ("repeat", k)


# ---- 6. the pool
def test_pool_calls_of_four_models_get_solo_bits(capi):
    who = [("pinhole", "d"), ("robomaster", "d"), ("tum", "d"), ("robomaster", "w1")]
    wins = [_window(capi, ws.pinhole_twin(n, 0) if m == "pinhole" else ws.case(m, n)[0], model=m) for m, n in who]
    solo = [_run(capi, [w])[0] for w in wins]
    pool = capi.BaPool(max_batch=4, window_us=20000)      # (a full batch does not sit out the window)
    out, sizes = [None] * 4, [0] * 4
    start = threading.Barrier(4)

    def agent(t):
        b = capi.BaWindowBatch([wins[t]])
        start.wait()
        res, n = pool.optimize(b)
        out[t], sizes[t] = _copy(res), n
    th = [threading.Thread(target=agent, args=(t,)) for t in range(4)]
    for x in th: x.start()
    for x in th: x.join()
    pool.close()
    print("batch sizes:", sizes)
    for t in range(4):
        assert out[t] is not None and _same_bits(out[t], solo[t]), who[t]
    assert all(1 <= n <= 4 for n in sizes)
    for n in set(sizes):                                  # the calls that report n rode in batches of n
        assert sizes.count(n) % n == 0, sizes


# ---- 7. the edges of the contract
def test_31_free_cameras_is_capacity_before_anything_runs(capi):
    big = ws.scene("robomaster", ws.OVER_CAPACITY, 0)
    small = ws.pinhole_twin("a", 0)
    for wins in ([_window(capi, big, model="robomaster")], [_window(capi, small, model="pinhole"), _window(capi, big, model="robomaster")]):
        batch = capi.BaWindowBatch(wins)
        for o in batch.outs:
            o["poses"][:] = 7.0
        with pytest.raises(capi.DvmError) as ei:
            batch.run(fast=True)
        assert ei.value.code == DVM_ERR_CAPACITY
        assert all(np.all(o["poses"] == 7.0) for o in batch.outs)


def test_bad_model_anywhere_is_invalid_and_writes_nothing(capi):
    sc = ws.case("robomaster", "a")[0]
    good = list(ks.MODELS["robomaster"])
    for bad in (capi.CameraModel.make(7, good), capi.CameraModel.make(1, [0.0] + good[1:]), capi.CameraModel.make(0, [400.0, 0.0, 480.0, 270.0])):
        batch = capi.BaWindowBatch([_window(capi, sc, model="robomaster") for _ in range(3)])
        batch.models[2] = bad
        for o in batch.outs:
            o["poses"][:] = 7.0; o["points"][:] = 7.0
        with pytest.raises(capi.DvmError) as ei:
            batch.run(fast=True)
        assert ei.value.code == DVM_ERR_INVALID
        assert all(np.all(o["poses"] == 7.0) and np.all(o["points"] == 7.0) for o in batch.outs)


def test_no_iterations_and_no_edges_inside_a_mixed_call(capi):
    fish, pin = ws.case("tum", "d")[0], ws.pinhole_twin("d", 0)
    none = dict(_window(capi, fish, model="tum"), edges=np.zeros(0, bs.EDGE_DTYPE))
    wins = [_window(capi, pin, model="pinhole"), _window(capi, fish, model="tum", iterations=0), _window(capi, fish, model="tum"), none,
            _window(capi, pin, model="pinhole", iterations=0)]
    a = _run(capi, wins)
    b = _run(capi, wins)
    plain = _run(capi, [wins[0], wins[2]])
    assert _same_bits(a[0], plain[0]) and _same_bits(a[2], plain[1]) and a[2]["stats"]["iterations"] >= 3
    for k in (1, 3, 4):
        if k != 3:      # (the window without edges has iterations to run: an empty problem's, which move nothing)
            assert a[k]["stats"]["iterations"] == 0 and a[k]["stats"]["total_trials"] == 0, k
        assert np.array_equal(_bits(a[k]["points"]), _bits(wins[k]["points"])), k
        assert float(np.abs(a[k]["poses"] - bs.normalize_all(wins[k]["poses"])).max()) <= 4e-16, k      # (SE3Quat's constructor normalises)
    # the window without iterations reports the chi2 of its input state: the restatement's residuals there
    pj, _ = bs.kb8_camera(ks.MODELS["tum"])
    Xc = bs._camera_frame_points(bs.normalize_all(fish["poses0"]), fish["points0"], fish["edges"])
    e = np.stack([fish["edges"]["u"], fish["edges"]["v"]], axis=1) - pj(Xc)
    chi0 = fish["edges"]["inv_sigma2"] * (e[:, 0] ** 2 + e[:, 1] ** 2)
    assert np.allclose(a[1]["edge_chi2"], chi0, rtol=1e-3, atol=1e-3)          # (theta's float ulp: some 1e-5 px on residuals of pixels)
    for k in range(len(wins)):                                                 # two runs give the same bits
        assert _same_bits(a[k], b[k]), k


# ---- 8. the fisheye windows were not solved as pinhole ones
def test_fisheye_window_is_not_its_pinhole_reading(capi):
    fish = ws.case("robomaster", "d")[0]
    as_kb8 = _run(capi, [_window(capi, fish, model="robomaster")])[0]
    as_pin = _run(capi, [dict(_window(capi, fish), model=capi.CameraModel.make(0, ks.MODELS["robomaster"][:4]))])[0]
    assert float(np.abs(as_pin["poses"] - as_kb8["poses"]).max()) > 1e-3
