"""dvm_fuse_targets_set_resident: the Fuse chain on targets that live in a dvm_keyframe_store.  The search kernels read the same arrays
in the same order as after dvm_fuse_targets_set_cam, so every comparison is array_equal against set_cam + run / run_hits on the same
keyframes: both forms, both camera models, mixed targets, masks, an empty target, slots in descending order and put in two calls, one
slot under two poses.  Then the ordering against put (no host synchronisation in between), the generation rule (DVM_ERR_STATE after a
put or a remove to a named slot) and the upload counters."""
import numpy as np
import pytest

import fuse_cam_scene as fcs
import fuse_targets_scene as fts
import kb8_scene as ks

pytestmark = pytest.mark.gpu

N_PTS = 200
SLOT_KEYPOINTS = fts.BIG_TARGET_KEYPOINTS
STATE, INVALID, CAPACITY = -6, -1, -3


def _putable(kf):
    """The keyframe dict as the store takes it: all three level tables (the Fuse chain reads two of them)."""
    if kf.get("level_sigma2") is None:
        kf = dict(kf, level_sigma2=(np.float32(1.0) / np.asarray(kf["inv_level_sigma2"], np.float32)).astype(np.float32))
    return kf


def _pose(kf):
    return (kf["Tcw"], kf["Ow"]) if kf.get("Ow") is not None else kf["Tcw"]


def _case(capi, kind, T):
    """(targets as FuseTargets.set takes them, models or None, forms or None, pts, skip, th)"""
    if kind == "pinhole":
        sc = fts.prefix(fts.scene(fcs.SEED_OF_T[T], T), N_PTS)
        return sc["targets"], None, None, sc["pts"], sc["skip"], 3.0
    if kind == "scw":
        sc = fcs.scw_scene(T)
        pts = {k: v for k, v in sc["pts"].items() if k not in ("id", "bad")}
        return [fcs.chain_target(kf) for kf in sc["targets"]], None, [1] * T, pts, sc["skip"], fcs.TH
    if kind in ks.MODELS:
        sc = fcs.kb8_scene(kind, T, N_PTS)
        return [fcs.kb8_chain_target(tg) for tg in sc["targets"]], [capi.CameraModel.make(1, ks.MODELS[kind])] * T, [t % 2 for t in range(T)], sc["pts"], sc["skip"], fcs.KB8_TH
    assert kind == "mixed"                         # pinhole and KannalaBrandt8 targets, both forms, over the pinhole scene's points
    sc = fts.prefix(fts.scene(fcs.SEED_OF_T[T], T), N_PTS)
    kb = fcs.kb8_scene("robomaster", T, N_PTS)
    tg, models, forms = [], [], []
    for t in range(T):
        if t % 2 == 0:
            tg.append(sc["targets"][t]); models.append(capi.CameraModel.pinhole(*sc["targets"][t]["K"]))
        else:
            tg.append(fcs.kb8_chain_target(kb["targets"][t])); models.append(capi.CameraModel.make(1, ks.MODELS["robomaster"]))
        forms.append((t // 2) % 2)
    if T == 1:
        tg.append(fcs.kb8_chain_target(kb["targets"][0])); models.append(capi.CameraModel.make(1, ks.MODELS["robomaster"])); forms.append(1)
    return tg, models, forms, sc["pts"], np.concatenate([sc["skip"]] * 2)[:len(tg)], 3.0


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.FuseTargets()
    h.reserve(N_PTS, 8, 5 * 700 + SLOT_KEYPOINTS)
    h.reserve_hits(8 * N_PTS)
    yield h
    h.close()


@pytest.fixture(scope="module")
def resident_chain(capi):
    """A handle that never holds uploaded targets: no max_total_target_keypoints."""
    h = capi.FuseTargets()
    h.reserve(N_PTS, 8, 0)
    h.reserve_hits(8 * N_PTS)
    yield h
    h.close()


def _rows(h, pts, skip, th):
    out = []
    for sk in (None, skip):
        bi, bd = h.run(pts, th, sk)
        off, hits = h.run_hits(pts, th, sk)
        out.append((bi, bd, off, hits))
    return out


def _assert_equal_rows(got, want):
    for g, w in zip(got, want):
        for a, b, name in zip(g, w, ("best_idx", "best_dist", "hit_off", "hits")):
            assert np.array_equal(a, b), name


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("kind", ["pinhole", "scw", "robomaster", "tum", "mixed"])
def test_rows_equal_the_uploaded_call(capi, chain, resident_chain, kind, T):
    tg, models, forms, pts, skip, th = _case(capi, kind, T)
    n_t = len(tg)
    chain.set(tg, models=models, forms=forms)
    want = _rows(chain, pts, skip, th)
    assert (want[0][0] >= 0).sum() >= (5 if kind != "mixed" else 1)
    if T == 5:
        assert any(len(kf["kps"]) == 0 for kf in tg)                                     # a target with n = 0
    # slots in descending order with gaps; the keyframes put in two separate calls
    store = capi.KeyframeStore(2 * n_t + 1, SLOT_KEYPOINTS)
    slots = [2 * (n_t - 1 - t) + 1 for t in range(n_t)]
    cut = n_t // 2
    store.put(slots[:cut], [_putable(kf) for kf in tg[:cut]])
    store.put(slots[cut:], [_putable(kf) for kf in tg[cut:]])
    for h in (chain, resident_chain):
        h.set_resident(store, slots, [_pose(kf) for kf in tg], models=models, forms=forms)
        _assert_equal_rows(_rows(h, pts, skip, th), want)
    store.close()


def test_one_slot_under_two_poses(capi, chain, resident_chain):
    sc = fts.prefix(fts.scene(fcs.SEED_OF_T[2], 2), N_PTS)
    kf = sc["targets"][0]
    other = dict(kf, Tcw=sc["targets"][1]["Tcw"])
    chain.set([kf, other, kf])
    want = _rows(chain, sc["pts"], np.concatenate([sc["skip"], sc["skip"][:1]]), 3.0)
    store = capi.KeyframeStore(3, 512)
    store.put([2], [kf])
    resident_chain.set_resident(store, [2, 2, 2], [kf["Tcw"], other["Tcw"], kf["Tcw"]])
    got = _rows(resident_chain, sc["pts"], np.concatenate([sc["skip"], sc["skip"][:1]]), 3.0)
    _assert_equal_rows(got, want)
    assert not np.array_equal(got[0][0][0], got[0][0][1]) and np.array_equal(got[0][0][0], got[0][0][2])
    store.close()


def test_put_then_set_and_run_without_a_host_synchronisation(capi, chain, resident_chain):
    """put returns before k_kfs_put has run; the run's stream waits for it (kfs_read_begin), nothing else orders the two."""
    tg, models, forms, pts, skip, th = _case(capi, "pinhole", 5)
    chain.set(tg)
    want = chain.run(pts, th, skip)
    store = capi.KeyframeStore(5, SLOT_KEYPOINTS)
    arr, keep = store.records([_putable(kf) for kf in tg])
    res = resident_chain.resident_targets(range(5), [_pose(kf) for kf in tg])
    slots = np.arange(5, dtype=np.int32)
    for _ in range(3):                                                                   # (each round overwrites the slots and bumps their generations)
        store.put_raw(slots, arr)
        resident_chain.set_resident_raw(store, res, 5)
        got = resident_chain.run(pts, th, skip)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    store.close()


def test_a_put_to_a_named_slot_invalidates_the_set(capi, chain, resident_chain):
    tg, _, _, pts, skip, th = _case(capi, "pinhole", 5)
    spare = fts.scene(fcs.SEED_OF_T[2], 2)["targets"][1]
    h = resident_chain
    store = capi.KeyframeStore(8, SLOT_KEYPOINTS)
    store.put(range(5), [_putable(kf) for kf in tg])
    poses = [_pose(kf) for kf in tg]
    h.set_resident(store, range(5), poses)
    first = h.run(pts, th, skip)
    store.put([6], [_putable(spare)])                                                    # a slot the set does not name: still valid
    again = h.run(pts, th, skip)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    store.put([3], [_putable(spare)])                                                    # a named one
    for run in (lambda: h.run(pts, th, skip), lambda: h.run_hits(pts, th, skip)):
        with pytest.raises(capi.DvmError) as e:
            run()
        assert e.value.code == STATE and "a target's slot was written since the set" in str(e.value)
    h.set_resident(store, range(5), poses)                                               # the handle stays usable: set again
    got = h.run(pts, th, skip)
    new_tg = list(tg); new_tg[3] = dict(spare, Tcw=tg[3]["Tcw"])
    chain.set(new_tg)
    want = chain.run(pts, th, skip)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(got[0][3], first[0][3])
    store.remove([0])                                                                    # a removed slot: the same rule, and no new set on it
    with pytest.raises(capi.DvmError) as e:
        h.run(pts, th, skip)
    assert e.value.code == STATE
    with pytest.raises(capi.DvmError) as e:
        h.set_resident(store, range(5), poses)
    assert e.value.code == INVALID and "target 0" in str(e.value)
    h.set_resident(store, range(1, 5), poses[1:])
    got = h.run(pts, th, skip[1:])
    assert np.array_equal(got[0], want[0][1:])
    store.close()


def test_errors_leave_the_handle_usable(capi, resident_chain):
    tg, _, _, pts, skip, th = _case(capi, "pinhole", 1)
    kb = fcs.kb8_chain_target(fcs.kb8_scene("robomaster", 1, N_PTS)["targets"][0])
    h = resident_chain
    store = capi.KeyframeStore(12, 1024)
    store.put([0, 1], [_putable(tg[0]), _putable(kb)])
    h.set_resident(store, [0], [_pose(tg[0])])
    want = h.run(pts, th, skip)
    for slots, models, code, word in (([5], None, INVALID, "never written"), ([12], None, INVALID, "slot 12"), ([-1], None, INVALID, "slot -1"),
                                      ([1], None, INVALID, "zero focal length"),            # the KannalaBrandt8 record carries no fx, fy
                                      ([0], [capi.CameraModel.make(2, ks.ROBOMASTER)], INVALID, "camera model"),
                                      ([0] * 9, None, CAPACITY, "9 targets")):
        with pytest.raises(capi.DvmError) as e:
            h.set_resident(store, slots, [_pose(tg[0])] * len(slots), models=models)
        assert e.value.code == code and word in str(e.value), (slots, str(e.value))
        got = h.run(pts, th, skip)                                                       # the earlier set is still there
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(capi.DvmError) as e:
        h.set_resident(store, [0], [_pose(tg[0])], forms=[2])
    assert e.value.code == INVALID
    store.close()


def test_upload_counters(capi, chain):
    """A resident set sends the target table alone: its bytes do not depend on the keypoints per target."""
    T = 5
    sets = {}
    for nk in (64, 1900):
        sc = fts.prefix(fts.scene(7, T, 200, nk), N_PTS)
        h = capi.FuseTargets()
        h.reserve(N_PTS, T, T * nk)
        h.set(sc["targets"])
        up_rows = h.run(sc["pts"], 3.0, sc["skip"])
        up_set, up_run = h.last_upload_bytes()
        store = capi.KeyframeStore(T, nk)
        store.put(range(T), [_putable(kf) for kf in sc["targets"]])
        h.set_resident(store, range(T), [_pose(kf) for kf in sc["targets"]])
        res_rows = h.run(sc["pts"], 3.0, sc["skip"])
        res_set, res_run = h.last_upload_bytes()
        assert np.array_equal(up_rows[0], res_rows[0]) and np.array_equal(up_rows[1], res_rows[1])
        assert res_run == up_run > N_PTS * 65                                            # the point table and the mask, either way
        assert up_set >= T * nk * 60 and 0 < res_set < up_set
        sets[nk] = res_set
        h.close(); store.close()
    assert sets[64] == sets[1900]
