"""dvm_create_new_map_points_cam on KannalaBrandt8 keyframes (tests/kb8_tri_scene.chain_scene) against the loop of the two _cam calls it
reschedules -- device against device, bit for bit -- and against its own host entry; model 0 through every _cam
entry against the pinhole entries on the pinhole scenes; and the refusals, which leave the handle usable."""
import numpy as np
import pytest

import kb8_scene as ks
import kb8_tri_scene as kt
import new_points_scene as nps

pytestmark = pytest.mark.gpu

VARIANTS = {"plain": dict(), "check_ori": dict(check_ori=True), "coarse": dict(coarse=True), "far": dict(far_points=True, th_far=9.0)}


def _model(capi, kf):
    return capi.CameraModel.make(capi.CameraModel.KANNALA_BRANDT8, kf["cam"])


def _models(capi, sc):
    return _model(capi, sc["cur"]), [_model(capi, kf) for kf in sc["neighbours"]]


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.NewPoints()
    h.reserve(2048, 30, 30 * 1024)
    yield h
    h.close()


def _run(capi, h, sc, **kw):
    cm, nm = _models(capi, sc)
    return h.create_new_map_points_cam(sc["cur"], sc["neighbours"], sc["median_depth"], cm, nm, **kw)


def _separate_calls(capi, sc, coarse=False, check_ori=False, cos_parallax_max=0.9998, far_points=False, th_far=0.0):
    """Per neighbour capi.search_for_triangulation_cam, then capi.triangulate_matches_cam, the table updated in between."""
    cur, nbs = sc["cur"], sc["neighbours"]
    cm, nm = _models(capi, sc)
    va = capi.keyframe_view(cur)                                   # (the view reads cur["mp"] in place)
    T1, Ow1 = nps.pose_3x4(cur["Tcw"])
    rf = np.float32(1.5) * np.float32(cur["scale_factors"][1])
    n_nb = len(nbs)
    out = dict(nb_status=np.zeros(n_nb, np.int32), nb_matches=np.zeros(n_nb, np.int32), pair_off=np.zeros(n_nb + 1, np.int32),
               new_point=np.full(len(cur["kps"]), -1, np.int32))
    P, S, Xs = [np.zeros((0, 2), np.int32)], [np.zeros(0, np.int32)], [np.zeros((0, 3), np.float32)]
    base = 0
    for j, nb in enumerate(nbs):
        out["pair_off"][j] = base
        T2, Ow2 = nps.pose_3x4(nb["Tcw"])
        if float(nps.baseline_ratio(Ow1, Ow2, sc["median_depth"][j])) < 0.01:
            out["nb_status"][j] = 1
            continue
        n, pairs = capi.search_for_triangulation_cam(va, capi.keyframe_view(nb), cm, nm[j], coarse, check_ori)
        out["nb_matches"][j] = n
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        X, st = capi.triangulate_matches_cam(cm, nm[j], T1, T2, Ow1, Ow2, cur["kps"], nb["kps"], pairs, cur["level_sigma2"], nb["level_sigma2"],
                                             cur["scale_factors"], nb["scale_factors"], rf, cos_parallax_max=cos_parallax_max, far_points=far_points, th_far=th_far)
        ok = np.nonzero(st == 0)[0]
        out["new_point"][pairs[ok, 0]] = base + ok
        cur["mp"][pairs[ok, 0]] = nps.NEW_POINT_ID
        P.append(pairs); S.append(st); Xs.append(X)
        base += len(pairs)
    out["pair_off"][n_nb] = base
    out.update(pairs=np.concatenate(P), status=np.concatenate(S), x3D=np.concatenate(Xs))
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", [1, 5, 30])
def test_chain_equals_the_loop_of_the_two_cam_calls(capi, chain, n, variant):
    seed = n % 2
    got = _run(capi, chain, nps.prefix(kt.chain_scene(seed), n), **VARIANTS[variant])
    want = _separate_calls(capi, nps.prefix(kt.chain_scene(seed), n), **VARIANTS[variant])
    nps.assert_same(got, want)
    if n >= 5:
        assert (got["nb_status"] == 1).sum() >= 1 and (got["status"] == 0).sum() >= 60 and len(got["pairs"]) > 100
    if n == 30:
        assert got["nb_matches"][nps.NO_SHARED_NODE] == 0 and got["nb_status"][nps.NEGATIVE_DEPTH] == 1 and got["nb_matches"][nps.OTHER_PYRAMID] > 10
    if variant == "far":
        assert (got["status"] == 8).sum() >= 1


def test_constraint_decides_and_the_fisheye_is_not_the_pinhole(capi, chain):
    """The constraint rejects what a coarse search takes, and the same keyframes read as pinhole cameras of p[0..3] give other points."""
    sc = nps.prefix(kt.chain_scene(0), 5)
    plain, coarse = _run(capi, chain, sc), _run(capi, chain, sc, coarse=True)
    assert coarse["nb_matches"].sum() > plain["nb_matches"].sum()
    pin = chain.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"])
    assert (pin["status"] == 0).sum() > 0 and not np.array_equal(plain["x3D"][:50], pin["x3D"][:50])


@pytest.mark.parametrize("n,variant", [(30, "check_ori"), (5, "plain"), (0, "plain")])
def test_host_entry_and_reuse(capi, chain, n, variant):
    sc = nps.prefix(kt.chain_scene(0), n)
    cm, nm = _models(capi, sc)
    dev = _run(capi, chain, sc, **VARIANTS[variant])
    host = capi.create_new_map_points_cam(sc["cur"], sc["neighbours"], sc["median_depth"], cm, nm, **VARIANTS[variant])
    nps.assert_same(host, dev)
    # a smaller problem on the same handle, then the first again: no stale rows
    small = _run(capi, chain, nps.prefix(kt.chain_scene(1), 5), check_ori=True)
    nps.assert_same(small, _separate_calls(capi, nps.prefix(kt.chain_scene(1), 5), check_ori=True))
    again = _run(capi, chain, sc, **VARIANTS[variant])
    for k in dev:
        assert dev[k].tobytes() == again[k].tobytes(), k


def test_model_0_through_every_cam_entry_is_the_pinhole_entry(capi, chain):
    for seed, n, variant in [(0, 30, "plain"), (1, 5, "check_ori"), (0, 5, "coarse"), (1, 5, "far")]:
        sc = nps.prefix(nps.scene(seed), n)
        cm = capi.CameraModel.pinhole(*sc["cur"]["K"]); nm = [capi.CameraModel.pinhole(*kf["K"]) for kf in sc["neighbours"]]
        want = chain.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"], **VARIANTS[variant])
        nps.assert_same(chain.create_new_map_points_cam(sc["cur"], sc["neighbours"], sc["median_depth"], cm, nm, **VARIANTS[variant]), want)
        nps.assert_same(capi.create_new_map_points_cam(sc["cur"], sc["neighbours"], sc["median_depth"], cm, nm, **VARIANTS[variant]), want)
        assert len(want["pairs"]) > 20
    # the search and the pair geometry, model 0: neighbour OTHER_PYRAMID has another K and another pyramid
    sc = nps.prefix(nps.scene(0), 5)
    va = capi.keyframe_view(sc["cur"])
    for j in (0, nps.OTHER_PYRAMID):
        nb = sc["neighbours"][j]
        vb = capi.keyframe_view(nb)
        cm = capi.CameraModel.pinhole(*sc["cur"]["K"]); nm = capi.CameraModel.pinhole(*nb["K"])
        for coarse in (False, True):
            n0, p0 = capi.search_for_triangulation(va, vb, coarse, True)
            n1, p1 = capi.search_for_triangulation_cam(va, vb, cm, nm, coarse, True)
            assert n0 == n1 and np.array_equal(p0, p1) and n0 > 10
        for a, b in zip(capi.triangulation_geometry(va, vb), capi.triangulation_geometry_cam(va, vb, cm, nm)):
            assert a.tobytes() == b.tobytes()


def test_refusals_leave_the_handle_usable(capi):
    h = capi.NewPoints()
    h.reserve(1024, 5, 5 * 1024)
    sc = nps.prefix(kt.chain_scene(1), 5)
    cm, nm = _models(capi, sc)
    want = _run(capi, h, sc)

    def refused(cur_model, nb_models):
        with pytest.raises(capi.DvmError) as e:
            h.create_new_map_points_cam(sc["cur"], sc["neighbours"], sc["median_depth"], cur_model, nb_models)
        assert e.value.code == -1, str(e.value)
        nps.assert_same(_run(capi, h, sc), want)                   # ... and the next call is served

    pin = capi.CameraModel.pinhole(*sc["cur"]["cam"][:4])
    refused(cm, nm[:2] + [pin] + nm[3:])                            # a mixed pair
    refused(pin, nm)
    refused(None, nm)                                               # a NULL model
    refused(cm, None)
    refused(cm, nm[:4] + [capi.CameraModel.make(2, ks.ROBOMASTER)])             # a model of 2
    refused(cm, [capi.CameraModel.make(1, np.r_[0.0, ks.ROBOMASTER[1:]])] + nm[1:])   # a zero focal length
    refused(capi.CameraModel.make(1, np.r_[ks.ROBOMASTER[:1], 0.0, ks.ROBOMASTER[2:]]), nm)
    with pytest.raises(capi.DvmError) as e:                         # the pinhole call's refusals are this call's too
        h.create_new_map_points_cam(sc["cur"], sc["neighbours"], sc["median_depth"], cm, nm, record_cap=10)
    assert e.value.code == -3
    nps.assert_same(_run(capi, h, sc), want)
    h.close()
