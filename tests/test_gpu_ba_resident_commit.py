"""dvm_ba_resident's prepare step and dvm_ba_resident_commit (capi.BaResident): geometry, point_dirty and ow are bit-equal to the float32
numpy restatement (ba_resident_scene.prepare_ref) fed with the call's own poses, points, edge_chi2 and depth_positive; after commit the map
store holds exactly the prepared geometry on clean points and the bit-identical old record everywhere else; the ordering against read,
update and the next optimize; per-window commits on two map stores; the state errors; every refusal, each followed by a good call with
the records read before and after."""
import numpy as np
import pytest

import ba_resident_scene as brs
from test_ba_resident_scene import permuted

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, CAPACITY_ERR, STATE = -1, -3, -6


def check_prepare(sc, r, ow=None, with_ref=True, chi2_erase=brs.CHI2_ERASE):
    geom, dirty, centres, state = brs.prepare_ref(sc, r, ow=ow, with_ref=with_ref, chi2_erase=chi2_erase)
    assert r["ow"].tobytes() == centres.tobytes()
    assert np.array_equal(r["point_dirty"], dirty)
    assert r["geometry"].tobytes() == geom.tobytes(), np.flatnonzero((r["geometry"].view(np.uint32) != geom.view(np.uint32)).any(axis=1))
    return geom, dirty, state


def all_records(pl):
    return [pl.map_store.read(s) for s in pl.mp_slots]


def observers_scene(seed=1, noise=0.3):
    """points with 1, 2, 7 (and 3, 4, 5) observers, two without any; the ref edge first, last, on a free and on a fixed camera"""
    n_obs = np.array([1, 2, 7, 3, 4, 5, 7, 2] * 6 + [0, 0])
    sc = brs.make_window(seed, 8, len(n_obs), int(n_obs.sum()), 3, n_obs=n_obs, noise=noise, iterations=10)
    o, ref = sc["obs"], sc["ref_edge"].copy()
    kinds = set()
    for l in np.flatnonzero(n_obs >= 2):
        mine = np.flatnonzero(o["point"] == l)
        on_fixed = mine[sc["fixed"][o["pose"][mine]] == 1]; on_free = mine[sc["fixed"][o["pose"][mine]] == 0]
        want = l % 4
        if want == 0:
            ref[l] = mine[0]; kinds.add("first")
        elif want == 1:
            ref[l] = mine[-1]; kinds.add("last")
        elif want == 2 and len(on_free):
            ref[l] = on_free[0]; kinds.add("free")
        elif want == 3 and len(on_fixed):
            ref[l] = on_fixed[0]; kinds.add("fixed")
    assert kinds == {"first", "last", "free", "fixed"}
    return dict(sc, ref_edge=ref), n_obs


def test_prepare_equals_the_restatement_and_commit_writes_exactly_it():
    from dvm_slam_amd import capi
    sc, n_obs = observers_scene()
    pl = brs.Placed([sc])
    before = all_records(pl)[0]
    h = capi.BaResident()
    r = h.optimize(pl.problems())[0]
    geom, dirty, state = check_prepare(sc, r)
    assert dirty.sum() == 0 and (state[n_obs == 0] == 2).all() and (state[n_obs > 0] == 0).all()      # no point dirty, as constructed
    for n in (1, 2, 7):
        assert (state[n_obs == n] == 0).any()
    assert all_records(pl)[0].tobytes() == before.tobytes()          # optimize alone writes nothing
    h.commit()                                                        # optimize -> commit -> read
    after = all_records(pl)[0]
    assert after.tobytes() == brs.committed_records(before, geom, state).tobytes()
    assert after[state == 2].tobytes() == before[state == 2].tobytes()
    for f in ("desc", "n_obs", "bad"):
        assert np.array_equal(after[f], before[f])
    assert (after["pos"][state == 0] != before["pos"][state == 0]).any()
    up, down = h.last_bytes()
    assert 12 * sc["E"] + 4 * sc["L"] < up < 200 * sc["E"] + (1 << 16) and down > 0
    h.close()


def test_camera_centres_given_for_the_fixed_cameras():
    from dvm_slam_amd import capi
    sc, _ = observers_scene(2)
    own = brs.camera_centres(sc["poses"], sc["poses"], np.ones(sc["P"], np.uint8))
    ow = (own + F32(1e-3)).astype(F32)
    ow[sc["fixed"] == 0] = np.nan                                     # rows of free cameras are not read
    pl = brs.Placed([sc], ow=[ow])
    h = capi.BaResident()
    r = h.optimize(pl.problems())[0]
    geom, _, state = check_prepare(sc, r, ow=ow)
    assert np.isfinite(r["ow"]).all() and np.array_equal(r["ow"][sc["fixed"] == 1], ow[sc["fixed"] == 1])
    absent = brs.prepare_ref(sc, r)[0]
    assert (absent.view(np.uint32) != geom.view(np.uint32)).any()    # the given rows are what the normals were taken from
    h.close()


def test_the_callers_edge_order_is_the_order_of_the_normals_sum():
    from dvm_slam_amd import capi
    sc = brs.make_window(21, 8, 30, 210, 2, noise=0.3, iterations=10)
    sp, perm = permuted(sc, np.random.default_rng(1))
    h = capi.BaResident()
    r0 = h.optimize(brs.Placed([sc]).problems())[0]
    g0, _, s0 = check_prepare(sc, r0)
    r1 = h.optimize(brs.Placed([sp]).problems())[0]
    g1, _, s1 = check_prepare(sp, r1)
    assert (s0 == 0).sum() >= 20 and np.array_equal(s0, s1)
    # the permuted call returns the permuted-order value (check_prepare above), and not the other order's: the restatement in the
    # ORIGINAL edge order, fed with the same call's results, differs in some normal's bits
    inv = np.argsort(perm)
    back = dict(r1, edge_chi2=r1["edge_chi2"][inv], depth_positive=r1["depth_positive"][inv])
    other = brs.prepare_ref(sc, back)[0]
    assert np.array_equal(other[:, :3], g1[:, :3]) and np.array_equal(other[:, 6:], g1[:, 6:])
    assert (other[:, 3:6].view(np.uint32) != g1[:, 3:6].view(np.uint32)).any()
    assert np.abs(g0 - g1).max() < 1e-3
    h.close()


def moved_scene():
    """four points with at least four observers get ONE keypoint moved by 30 px in its keyframe"""
    sc, n_obs = observers_scene(3)
    kfs = [dict(kf, kps=kf["kps"].copy()) for kf in sc["kfs"]]
    victims = np.flatnonzero(n_obs >= 4)[:4]
    for l in victims:
        e = np.flatnonzero(sc["obs"]["point"] == l)[1]
        kfs[sc["obs"]["pose"][e]]["kps"]["x"][sc["obs"]["kp"][e]] += F32(30.0)
    return dict(sc, kfs=kfs), victims


def test_dirty_points_keep_their_records():
    from dvm_slam_amd import capi
    h = capi.BaResident()
    # (a) a keypoint moved 30 px
    sc, victims = moved_scene()
    pl = brs.Placed([sc])
    before = all_records(pl)[0]
    r = h.optimize(pl.problems())[0]
    assert np.array_equal(np.flatnonzero(r["point_dirty"]), victims)           # the flags as constructed, first
    geom, dirty, state = check_prepare(sc, r)
    h.commit()                                                                  # commit -> update (of the dirty points) -> read
    rebuilt = before[victims].copy(); rebuilt["bad"] = 1; rebuilt["n_obs"] -= 1
    pl.map_store.update(pl.mp_slots[0][victims], rebuilt)
    after = all_records(pl)[0]
    want = brs.committed_records(before, geom, state); want[victims] = rebuilt
    assert after.tobytes() == want.tobytes()
    # (b) points behind a camera
    sc = brs.make_window(31, 5, 40, 150, 2, behind=3, noise=0.3, iterations=10)
    pl = brs.Placed([sc])
    before = all_records(pl)[0]
    r = h.optimize(pl.problems())[0]
    assert np.array_equal(np.flatnonzero(r["point_dirty"]), [37, 38, 39]) and (r["depth_positive"] == 0).sum() == 3            # the flags as constructed, first
    geom, dirty, state = check_prepare(sc, r)
    h.commit()
    after = all_records(pl)[0]
    assert after.tobytes() == brs.committed_records(before, geom, state).tobytes() and after[37:].tobytes() == before[37:].tobytes()
    # (c) every point dirty: nothing is written
    pr = [dict(p, chi2_erase=-1.0) for p in pl.problems()]
    before = after
    r = h.optimize(pr)[0]
    assert r["point_dirty"].all()
    check_prepare(sc, r, chi2_erase=-1.0)
    assert (r["geometry"] == 0).all()
    h.commit()
    assert all_records(pl)[0].tobytes() == before.tobytes()
    h.close()


def test_commit_then_optimize_with_nothing_in_between():
    """the second optimize reads the committed positions and must not overwrite what the queued commit still reads"""
    from dvm_slam_amd import capi
    sc, _ = observers_scene(4)
    other = brs.make_window(41, 4, 300, 900, 2, noise=0.3)
    pl = brs.Placed([sc]); po = brs.Placed([other])
    before = all_records(pl)[0]
    h = capi.BaResident()
    r = h.optimize(pl.problems())[0]
    geom, _, state = brs.prepare_ref(sc, r)[0], None, brs.prepare_ref(sc, r)[3]
    h.commit()
    r2 = h.optimize(po.problems() + pl.problems())
    want = brs.committed_records(before, geom, state)
    assert all_records(pl)[0].tobytes() == want.tobytes()
    sc2 = dict(sc, records=want)
    up = capi.ba_optimize_windows([brs.host_window(sc2)], fast=True)[0]
    assert np.array_equal(r2[1]["points"].view(np.uint64), up["points"].view(np.uint64)) and np.array_equal(r2[1]["poses"].view(np.uint64), up["poses"].view(np.uint64))
    check_prepare(sc2, r2[1]); check_prepare(other, r2[0])
    h.close()


def test_per_window_commits_on_two_map_stores_and_the_state_errors():
    from dvm_slam_amd import capi
    a = [brs.make_window(50 + k, 4, 40, 130, 2, noise=0.3) for k in range(2)]
    b = [brs.make_window(55, 5, 50, 170, 2, noise=0.3)]
    pa, pb = brs.Placed(a), brs.Placed(b)
    pr = [pa.problems()[0], pb.problems()[0], pa.problems()[1]]
    scenes = [a[0], b[0], a[1]]
    h = capi.BaResident()

    def state_error(k):
        with pytest.raises(capi.DvmError) as e:
            h.commit(k)
        assert e.value.code == STATE, k
    state_error(-1); state_error(0)                                   # before any optimize
    before = [all_records(pa)[0], all_records(pb)[0], all_records(pa)[1]]
    res = h.optimize(pr)
    prep = [check_prepare(s, r) for s, r in zip(scenes, res)]
    want = [brs.committed_records(bf, g, st) for bf, (g, _, st) in zip(before, prep)]
    now = lambda: [all_records(pa)[0], all_records(pb)[0], all_records(pa)[1]]     # noqa: E731

    def holds(done):
        for k, rec in enumerate(now()):
            assert rec.tobytes() == (want[k] if k in done else before[k]).tobytes(), (k, done)
    h.commit(1); holds({1})
    state_error(1)                                                    # a second commit of the same window
    h.commit(0); holds({0, 1})
    h.commit(-1); holds({0, 1, 2})
    h.commit(-1)                                                      # nothing left: not an error
    state_error(2)
    with pytest.raises(capi.DvmError) as e:
        h.commit(3)
    assert e.value.code == INVALID
    # a window without ref_edge cannot be committed; min_dist / max_dist are zeros
    res = h.optimize([dict(pr[0], ref_edge=None), pr[1]])
    check_prepare(scenes[0], res[0], with_ref=False)
    state_error(0)
    h.commit(-1)                                                      # commits window 1 alone
    state_error(1)
    # after an optimize that failed
    with pytest.raises(capi.DvmError) as e:
        h.optimize([dict(pr[0], mp_slots=pr[0]["mp_slots"] * 0 - 1)])
    assert e.value.code == INVALID
    state_error(-1); state_error(0)
    h.close()


def test_every_refusal_leaves_the_stores_and_the_handle_as_they_were():
    from dvm_slam_amd import capi
    sc = brs.make_window(60, 4, 40, 130, 2, noise=0.3)
    pl = brs.Placed([sc])
    pr = pl.problems()[0]
    h = capi.BaResident()
    before = all_records(pl)[0]
    good = h.optimize([pr])[0]
    good = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
    E, L, P = sc["E"], sc["L"], sc["P"]

    def ch(key, idx, val, field=None):
        a = pr[key].copy()
        if field:
            a[field][idx] = val
        else:
            a[idx] = val
        return dict(pr, **{key: a})
    used = np.flatnonzero(np.bincount(sc["obs"]["point"], minlength=L) > 0)
    l0 = int(used[0])
    not_mine = int(np.flatnonzero(sc["obs"]["point"] != l0)[0])
    cap_kf, cap_mp = pl.kf_store.capacity, pl.map_store.capacity
    n_kp = len(sc["kfs"][sc["obs"]["pose"][5]]["kps"])
    bad_model = capi.CameraModel.make(0, [0.0, 510.0, 320.0, 240.0])
    cases = [
        ("keyframe slot outside the store", INVALID, ch("kf_slots", 1, cap_kf)),
        ("negative keyframe slot", INVALID, ch("kf_slots", 1, -1)),
        ("keyframe slot never written", INVALID, ch("kf_slots", 1, 0)),
        ("kp = n of its slot", INVALID, ch("obs", 5, n_kp, "kp")),
        ("kp negative", INVALID, ch("obs", 5, -1, "kp")),
        ("map slot out of range", INVALID, ch("mp_slots", 3, cap_mp)),
        ("map slot never written", INVALID, ch("mp_slots", 3, 0)),
        ("map slot twice", INVALID, ch("mp_slots", 3, pr["mp_slots"][7])),
        ("ref_edge out of range", INVALID, ch("ref_edge", l0, E)),
        ("ref_edge not an edge of its point", INVALID, ch("ref_edge", l0, not_mine)),
        ("ref_edge -1 on a point that has edges", INVALID, ch("ref_edge", l0, -1)),
        ("edge's pose out of range", INVALID, ch("obs", 9, P, "pose")),
        ("edge's point out of range", INVALID, ch("obs", 9, L, "point")),
        ("edge's point negative", INVALID, ch("obs", 9, -1, "point")),
        ("invalid model", INVALID, dict(pr, model=bad_model)),
        ("model outside {0, 1}", INVALID, dict(pr, model=capi.CameraModel.make(2, list(brs.PINHOLE_K)))),
    ]
    assert not pl.kf_store is None and 0 not in pl.kf_slots[0] and 0 not in pl.mp_slots[0]
    big = brs.make_window(61, 33, 40, 600, 2)                          # 31 free cameras
    pbig = brs.Placed([big])
    cases.append(("more than 30 free cameras", CAPACITY_ERR, pbig.problems()[0]))
    if capi.device_count() > 1:
        far = brs.Placed([sc], kf_store=capi.KeyframeStore(cap_kf, 256, device=1), map_store=capi.MapStore(cap_mp, device=1))
        capi.MapStore(1, device=0).close()          # (the calling thread's current device is 0 again)
        cases.append(("keyframe store on another device", INVALID, dict(pr, keyframe_store=far.kf_store)))
        cases.append(("map store on another device", INVALID, dict(pr, map_store=far.map_store)))

    def good_again(what):
        assert all_records(pl)[0].tobytes() == before.tobytes(), what
        r = h.optimize([pr])[0]
        for key in ("poses", "points", "edge_chi2", "depth_positive", "geometry", "point_dirty", "ow"):
            assert r[key].tobytes() == good[key].tobytes(), (what, key)
    for what, code, bad in cases:
        batch = capi.BaResidentBatch([pr, bad])                        # the good window first: nothing of it may be written either
        with pytest.raises(capi.DvmError) as e:
            h.run(batch)
        assert e.value.code == code, what
        for o in batch.outs:
            assert all((v == 0).all() for v in o.values() if isinstance(v, np.ndarray)), what     # no output written
        good_again(what)
    # NULL arrays
    for field in ("poses", "fixed", "keyframes", "kf_slot", "points", "mp_slot", "obs"):
        batch = capi.BaResidentBatch([pr])
        setattr(batch.wins[0], field, None)
        with pytest.raises(capi.DvmError) as e:
            h.run(batch)
        assert e.value.code == INVALID, field
        good_again("NULL " + field)
    with pytest.raises(capi.DvmError) as e:
        capi.check(h.L.dvm_ba_resident_optimize(h.h, None, None, 1, None, None))
    assert e.value.code == INVALID
    # a keyframe slot that has been removed
    pl.kf_store.remove(pl.kf_slots[0][2:3])
    with pytest.raises(capi.DvmError) as e:
        h.optimize([pr])
    assert e.value.code == INVALID
    pl.kf_store.put(pl.kf_slots[0][2:3], sc["kfs"][2:3])
    good_again("removed slot put again")
    h.commit()                                                         # and the handle still commits
    assert all_records(pl)[0].tobytes() == brs.committed_records(before, good["geometry"], brs.prepare_ref(sc, good)[3]).tobytes()
    h.close()
