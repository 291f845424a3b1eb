"""dvm_create_new_map_points_resident: CreateNewMapPoints on keyframes that live in a dvm_keyframe_store.  The kernels are the uploaded
call's and read the same arrays, so every comparison is new_points_scene.assert_same (x3D bit for bit) against dvm_create_new_map_points
/ _cam on the same keyframes: 1 and 5 neighbours (one skipped by the baseline test), a KannalaBrandt8 chain scene, a second call with a
changed mvpMapPoints on the same slots, and the error paths."""
import numpy as np
import pytest

import kb8_tri_scene as kt
import new_points_scene as nps

pytestmark = pytest.mark.gpu

SLOT_KEYPOINTS = 1024
INVALID, CAPACITY = -1, -3
VARIANTS = {"plain": dict(), "coarse_ori": dict(coarse=True, check_ori=True), "far": dict(far_points=True, th_far=9.0)}


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.NewPoints()
    h.reserve(2048, 30, 30 * 1024)
    yield h
    h.close()


def _put(capi, sc, cur_slot=None):
    """A store holding the scene: neighbours in descending slots, the current keyframe behind them."""
    n = len(sc["neighbours"])
    store = capi.KeyframeStore(n + 2, SLOT_KEYPOINTS)
    nb_slots = [n - j for j in range(n)]
    cur_slot = n + 1 if cur_slot is None else cur_slot
    store.put([cur_slot] + nb_slots, [sc["cur"]] + list(sc["neighbours"]))
    return store, cur_slot, nb_slots


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("seed", [0, 1])
def test_records_equal_the_uploaded_call(capi, chain, seed, n, variant):
    sc = nps.prefix(nps.scene(seed), n)
    want = chain.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"], **VARIANTS[variant])
    up_bytes = chain.last_upload_bytes()
    store, cs, ns = _put(capi, sc)
    got = chain.create_new_map_points_resident(store, cs, sc["cur"], ns, sc["neighbours"], sc["median_depth"], **VARIANTS[variant])
    nps.assert_same(got, want)
    assert len(got["pairs"]) >= 10
    if n == 5:
        assert got["nb_status"][nps.TINY_BASELINE[0]] == 1 and (got["nb_status"] == 0).sum() == 4     # one neighbour skipped by the baseline test
    # mvpMapPoints and the per-neighbour geometry travel, the keyframes do not: 4 B per keypoint against about 70
    res_bytes = chain.last_upload_bytes()
    kps = len(sc["cur"]["kps"]) + sum(len(kf["kps"]) for j, kf in enumerate(sc["neighbours"]) if got["nb_status"][j] == 0)
    assert 4 * kps <= res_bytes <= 4 * kps + 1024 * (n + 1) and up_bytes >= 60 * kps
    store.close()


@pytest.mark.parametrize("variant", ["plain", "coarse_ori"])
def test_kb8_chain_scene_equals_the_cam_call(capi, chain, variant):
    sc = nps.prefix(kt.chain_scene(0), 5)
    cm = capi.CameraModel.make(capi.CameraModel.KANNALA_BRANDT8, sc["cur"]["cam"])
    nm = [capi.CameraModel.make(capi.CameraModel.KANNALA_BRANDT8, kf["cam"]) for kf in sc["neighbours"]]
    want = chain.create_new_map_points_cam(sc["cur"], sc["neighbours"], sc["median_depth"], cm, nm, **VARIANTS[variant])
    store, cs, ns = _put(capi, sc)
    got = chain.create_new_map_points_resident(store, cs, sc["cur"], ns, sc["neighbours"], sc["median_depth"], cm, nm, **VARIANTS[variant])
    nps.assert_same(got, want)
    assert len(got["pairs"]) >= 10 and (got["status"] == 0).sum() >= 5
    # model 0 structs on the slots: the pinhole chain, as dvm_create_new_map_points_cam under model 0
    sp = nps.prefix(nps.scene(0), 5)
    pm = capi.CameraModel.pinhole(*sp["cur"]["K"]); pn = [capi.CameraModel.pinhole(*kf["K"]) for kf in sp["neighbours"]]
    want0 = chain.create_new_map_points(sp["cur"], sp["neighbours"], sp["median_depth"], **VARIANTS[variant])
    store0, cs0, ns0 = _put(capi, sp)
    nps.assert_same(chain.create_new_map_points_resident(store0, cs0, sp["cur"], ns0, sp["neighbours"], sp["median_depth"], pm, pn, **VARIANTS[variant]), want0)
    store.close(); store0.close()


def test_a_second_call_with_a_changed_table(capi, chain):
    """LocalMapping changes mvpMapPoints between two calls: mp travels per call, the slots stay as put."""
    sc = nps.prefix(nps.scene(1), 5)
    store, cs, ns = _put(capi, sc)
    first = chain.create_new_map_points_resident(store, cs, sc["cur"], ns, sc["neighbours"], sc["median_depth"])
    nps.assert_same(first, chain.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"]))
    # the first call's new points enter the current keyframe's table, and a neighbour loses some of its points
    cur2 = dict(sc["cur"]); cur2["mp"] = sc["cur"]["mp"].copy()
    made = first["pairs"][first["status"] == 0]
    cur2["mp"][made[:len(made) // 2, 0]] = nps.NEW_POINT_ID
    nb2 = list(sc["neighbours"])
    mp0 = nb2[0]["mp"].copy(); mp0[np.flatnonzero(mp0 >= 0)[::3]] = -1
    nb2[0] = dict(nb2[0], mp=mp0)
    sc2 = dict(cur=cur2, neighbours=nb2, median_depth=sc["median_depth"])
    want = chain.create_new_map_points(sc2["cur"], sc2["neighbours"], sc2["median_depth"])
    got = chain.create_new_map_points_resident(store, cs, sc2["cur"], ns, sc2["neighbours"], sc2["median_depth"])
    nps.assert_same(got, want)
    assert not np.array_equal(got["pairs"], first["pairs"])
    store.close()


def _empty_fv(kf):
    return dict(kf, fv=dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32)))


def test_a_keyframe_without_a_feature_vector_is_legal_and_matches_nothing(capi, chain):
    """fv_n = 0 as cur: legal, zero matches -- what dvm_create_new_map_points gives on a dvm_np_keyframe with fv_n = 0."""
    sc = nps.prefix(nps.scene(0), 5)
    bare = dict(sc, cur=_empty_fv(sc["cur"]))
    want = chain.create_new_map_points(bare["cur"], bare["neighbours"], bare["median_depth"])
    store, cs, ns = _put(capi, bare)
    got = chain.create_new_map_points_resident(store, cs, bare["cur"], ns, bare["neighbours"], bare["median_depth"])
    nps.assert_same(got, want)
    assert len(got["pairs"]) == 0 and (got["nb_matches"] == 0).all() and (got["new_point"] == -1).all() and (got["nb_status"] == 0).sum() == 4
    # and as a neighbour: that neighbour alone finds nothing
    nb = list(sc["neighbours"]); nb[2] = _empty_fv(nb[2])
    sc3 = dict(sc, neighbours=nb)
    store.put([ns[2]], [nb[2]])
    store.put([cs], [sc["cur"]])
    got = chain.create_new_map_points_resident(store, cs, sc3["cur"], ns, sc3["neighbours"], sc3["median_depth"])
    nps.assert_same(got, chain.create_new_map_points(sc3["cur"], sc3["neighbours"], sc3["median_depth"]))
    assert got["nb_matches"][2] == 0 and got["nb_matches"][0] > 0
    store.close()


def test_errors(capi, chain):
    sc = nps.prefix(nps.scene(0), 3)
    store, cs, ns = _put(capi, sc)
    args = (sc["cur"], ns, sc["neighbours"], sc["median_depth"])
    want = chain.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"])

    def refused(code, word, fn):
        with pytest.raises(capi.DvmError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), str(e.value)
        nps.assert_same(chain.create_new_map_points_resident(store, cs, *args), want)       # the handle stays usable
    refused(INVALID, "current keyframe: slot 0", lambda: chain.create_new_map_points_resident(store, 0, *args))          # never written
    refused(INVALID, "neighbour 1: slot 0", lambda: chain.create_new_map_points_resident(store, cs, sc["cur"], [ns[0], 0, ns[2]], *args[2:]))
    refused(INVALID, "slot 99", lambda: chain.create_new_map_points_resident(store, 99, *args))
    store.remove([ns[2]])
    with pytest.raises(capi.DvmError) as e:
        chain.create_new_map_points_resident(store, cs, *args)
    assert e.value.code == INVALID and "neighbour 2" in str(e.value)
    store.put([ns[2]], [sc["neighbours"][2]])
    # a missing mp, a record_cap below the bound, a neighbour of another pyramid length
    refused(INVALID, "missing keypoint array", lambda: chain.create_new_map_points_resident(store, cs, dict(sc["cur"], mp=None), *args[1:], record_cap=5000))
    refused(CAPACITY, "record_cap", lambda: chain.create_new_map_points_resident(store, cs, *args, record_cap=10))
    short = dict(sc["neighbours"][1], scale_factors=sc["neighbours"][1]["scale_factors"][:7], level_sigma2=sc["neighbours"][1]["level_sigma2"][:7],
                 inv_level_sigma2=sc["neighbours"][1]["inv_level_sigma2"][:7])
    short["kps"] = short["kps"].copy(); short["kps"]["octave"] = np.minimum(short["kps"]["octave"], 6)
    store.put([0], [short])
    with pytest.raises(capi.DvmError) as e:
        chain.create_new_map_points_resident(store, cs, sc["cur"], [ns[0], 0, ns[2]], *args[2:])
    assert e.value.code == INVALID and "level tables of another length" in str(e.value)
    small = capi.NewPoints()
    small.reserve(2048, 2, 2 * 1024)
    with pytest.raises(capi.DvmError) as e:
        small.create_new_map_points_resident(store, cs, *args)
    assert e.value.code == CAPACITY
    small.close(); store.close()
