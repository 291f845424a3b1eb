"""dvm_ba_resident_optimize (capi.BaResident): the cluster form of the window optimizer reading its observations from keyframe-store slots
and its points from map-store slots (k_ba_res_gather in front of the unchanged k_ba_window_cluster).  Every case is compared with
ba_optimize_windows(fast=True) on the window gathered on the host from the same keyframes and records (ba_resident_scene.host_window): the
same bits in poses, points, edge_chi2 and depth_positive, and every statistic except the times.  Every Placed() is update -> put ->
optimize with nothing in between."""
import numpy as np
import pytest

import ba_resident_scene as brs

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 255, 256, 257)
TIMES = ("ms_structure", "ms_optimize", "kernel_us")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(res, up, tag=""):
    assert len(res) == len(up)
    for k, (r, u) in enumerate(zip(res, up)):
        for key in ("poses", "points", "edge_chi2", "depth_positive"):
            assert r[key].shape == u[key].shape and np.array_equal(_bits(r[key]), _bits(u[key])), (tag, k, key)
        assert set(r["stats"]) == set(u["stats"])
        for key in r["stats"]:
            if key not in TIMES:
                a, b = r["stats"][key], u["stats"][key]
                assert np.array_equal(_bits(np.asarray(a, np.float64)), _bits(np.asarray(b, np.float64))), (tag, k, key, a, b)


def uploaded(capi, scenes, use_model=True, stop_flag=None):
    out = capi.ba_optimize_windows([brs.host_window(s, use_model) for s in scenes], fast=True, stop_flag=stop_flag)
    return [dict(o, poses=o["poses"].copy(), points=o["points"].copy(), edge_chi2=o["edge_chi2"].copy(), depth_positive=o["depth_positive"].copy()) for o in out]


def run(capi, scenes, use_model=True, stop_flag=None, **kw):
    pl = brs.Placed(scenes, use_model=use_model, **kw)
    h = capi.BaResident()
    res = h.optimize(pl.problems(), stop_flag=stop_flag)
    h.close(); pl.kf_store.close(); pl.map_store.close()
    return res


def edge_scenes():
    return [brs.make_window(100 + E, 4, 90, E, 2) for E in SIZES]


def point_scenes():
    return [brs.make_window(200 + L, 4, L, min(2 * L + 3, 4 * L), 2) for L in SIZES]


def test_edge_and_point_counts_around_the_block_sizes():
    """E and L at 1, 63, 64, 65, 255, 256, 257 (E = 1 with 90 points: 89 of them without an edge); camera 0's keyframe has kp = 0 and
    n - 1 and octaves 0 and n_levels - 1 in use, camera 2's has the other level tables (1.1, 5 levels); both stores' slots descend with gaps"""
    from dvm_slam_amd import capi
    for scenes in (edge_scenes(), point_scenes()):
        res = run(capi, scenes)
        same(res, uploaded(capi, scenes))
        assert max(r["stats"]["iterations"] for r in res) > 0


def special_scenes():
    return [brs.make_window(301, 3, 50, 120, 2),                                   # one free camera
            brs.make_window(302, 5, 64, 257, 2, twice=True, fixed_only=6, unused=5),   # a point seen twice by one camera, points seen by fixed cameras only, points without edges
            brs.make_window(303, 6, 80, 300, 3, outliers=0.1, iterations=10),
            brs.make_window(304, 2, 30, 0, 1)]                                     # no edge at all


def test_special_windows():
    from dvm_slam_amd import capi
    scenes = special_scenes()
    assert scenes[0]["fixed"].sum() == scenes[0]["P"] - 1
    same(run(capi, scenes), uploaded(capi, scenes))


@pytest.mark.parametrize("K", [1, 3, 9])
def test_window_counts(K):
    from dvm_slam_amd import capi
    scenes = [brs.make_window(400 + k, 3 + k % 4, 40 + 9 * k, 2 * (40 + 9 * k) + 10, 1 + k % 2) for k in range(K)]
    same(run(capi, scenes), uploaded(capi, scenes), f"K={K}")


def test_windows_of_one_call_on_two_keyframe_stores_and_two_map_stores():
    from dvm_slam_amd import capi
    a = [brs.make_window(500 + k, 4, 50, 160, 2) for k in range(2)]
    b = [brs.make_window(510 + k, 5, 70, 200, 2) for k in range(2)]
    pa, pb = brs.Placed(a), brs.Placed(b)
    pr = pa.problems() + pb.problems()
    order = [0, 2, 1, 3]                 # the stores interleave
    h = capi.BaResident()
    res = h.optimize([pr[i] for i in order])
    same(res, uploaded(capi, [(a + b)[i] for i in order]))
    h.close()


def model_scenes(capi):
    m = dict(pinhole=brs.pinhole(), robomaster=capi.CameraModel.robomaster(), tum=capi.CameraModel.tum())
    return {name: [brs.make_window(600 + k, 4, 60, 200, 2, model=mod) for k in range(2)] for name, mod in m.items()}


def test_camera_models_and_a_mixed_call():
    from dvm_slam_amd import capi
    sc = model_scenes(capi)
    for name, scenes in sc.items():
        same(run(capi, scenes), uploaded(capi, scenes), name)
    mixed = [sc["robomaster"][0], sc["pinhole"][0], sc["tum"][1], sc["pinhole"][1], sc["robomaster"][1]]
    res = run(capi, mixed)
    same(res, uploaded(capi, mixed), "mixed")
    # models NULL: the pinhole camera of cam, against dvm_ba_optimize_windows_fast with the same intrinsics
    same(run(capi, sc["pinhole"], use_model=False), uploaded(capi, sc["pinhole"], use_model=False), "no models")
    same(run(capi, sc["pinhole"], use_model=False), res[1:4:2], "model 0 is the pinhole window")


@pytest.mark.parametrize("G", [1, 2, 8])
def test_cluster_sizes(monkeypatch, G):
    from dvm_slam_amd import capi
    scenes = special_scenes()[:3]
    ref = uploaded(capi, scenes)
    monkeypatch.setenv("DVM_BA_CLUSTER", str(G))
    same(run(capi, scenes), ref, f"G={G}")


def test_repeat_after_a_barrier_timeout_runs_gather_and_prepare_again(monkeypatch):
    from dvm_slam_amd import capi
    scenes = special_scenes()[:3]
    ref = uploaded(capi, scenes)
    plain = run(capi, scenes)
    monkeypatch.setenv("DVM_BA_TEST_TIMEOUT", "1")
    res = run(capi, scenes)
    same(res, ref, "repeat")
    for r, p in zip(res, plain):
        for key in ("geometry", "point_dirty", "ow"):
            assert r[key].tobytes() == p[key].tobytes(), key


def test_private_tables(monkeypatch):
    from dvm_slam_amd import capi
    scenes = [brs.make_window(700 + k, 4, 50, 170, 2) for k in range(4)]
    ref = uploaded(capi, scenes)
    monkeypatch.setenv("DVM_BA_TEST_PRIVATE_TABLES", "1")
    same(run(capi, scenes), ref, "private tables")


def test_raised_stop_flag():
    from dvm_slam_amd import capi
    scenes = special_scenes()[:2]
    stop = np.ones(1, np.uint8)
    res = run(capi, scenes, stop_flag=stop)
    same(res, uploaded(capi, scenes, stop_flag=stop), "stop")
    free = run(capi, scenes)
    assert all(r["stats"]["iterations"] < f["stats"]["iterations"] for r, f in zip(res, free))
