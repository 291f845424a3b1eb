"""dvm_update_local_map_points: local_slot, n_local, frame_mp and n_outside against UpdateLocalPoints restated in tests/local_map_scene.py,
integer equality.  slot_keypoints 320 (two 256-entry blocks per row), keyframe capacity 140, map capacity 1 000; n_kfs of 1, 3, 81 and 129,
so the scan passes 256 workgroups; frame sizes 0 .. 1 025; batches of 1 and 3; a point first met in the last named keyframe; repeats inside
a row and across rows; local_cap one below the count with guard words behind the arrays; ordering behind dvm_map_store_update, a row patch,
dvm_ba_resident_commit and dvm_map_store_refresh with nothing synchronised by the test between; idle tables across calls and behind a
DVM_ERR_CAPACITY call; every refusal."""
import numpy as np
import pytest

import local_map_scene as lms

pytestmark = pytest.mark.gpu

SLOT_KEYPOINTS, KF_CAPACITY, MAP_CAPACITY = 320, 140, 1000
ROW_LENS = (320, 0, 1, 63, 64, 65, 257, 256, 255, 319, 3, 128)
FRAME_NS = (0, 1, 63, 64, 65, 257, 1025)
INVALID, CAPACITY_ERR = -1, -3


@pytest.fixture(scope="module")
def ulm(capi):
    u = capi.UpdateLocalMap()
    u.reserve(3, 1025, 129, MAP_CAPACITY, KF_CAPACITY, SLOT_KEYPOINTS)
    yield u
    u.close()


def _placed(capi, seed, n_live=130, **kw):
    rng = np.random.default_rng(seed)
    slots = np.sort(rng.permutation(KF_CAPACITY)[:n_live])
    lens = [ROW_LENS[(i + seed) % len(ROW_LENS)] for i in range(n_live)]
    a = dict(kf_slots=slots, row_lens=lens, n_points=800, frame_n=257, map_capacity=MAP_CAPACITY, kf_capacity=KF_CAPACITY,
             slot_keypoints=SLOT_KEYPOINTS, fill=0.5, queued=(1, 5))
    a.update(kw)
    return lms.Placed(capi, lms.make_graph(seed, **a))


@pytest.fixture(scope="module")
def big(capi):
    p = _placed(capi, 11)
    yield p
    p.close()


@pytest.fixture(scope="module")
def others(capi):
    ps = [_placed(capi, 12, n_live=9, n_points=300), _placed(capi, 13, n_live=40, n_points=500)]
    yield ps
    for p in ps:
        p.close()


def _order(p, n_kfs, seed=0):
    rng = np.random.default_rng(seed)
    return [p.g.kfs[i] for i in rng.permutation(len(p.g.kfs))[:n_kfs]]


def _check(res, g, order, local_cap=None):
    local, frame_mp, n_outside = lms.reference_points(g, order)
    cap = len(local) if local_cap is None else local_cap
    assert res["n_local"] == len(local) and res["n_outside"] == n_outside
    assert res["local_slot"].dtype == np.int32 and np.array_equal(res["local_slot"], local[:cap])
    assert np.array_equal(res["frame_mp"], frame_mp)
    assert (res["local_guarded"][min(cap, len(local)):] == -7).all() and (res["frame_mp_guarded"][len(frame_mp):] == -7).all()
    return local, frame_mp


@pytest.mark.parametrize("n_kfs", [1, 3, 81, 129])
def test_named_keyframes(ulm, big, n_kfs):
    order = _order(big, n_kfs, n_kfs)
    local, frame_mp = _check(ulm.points([big.frame_points(order)])[0], big.g, order)
    if n_kfs == 129:
        assert n_kfs * 2 > 256 and len(local) > 256                                  # two workgroups per row: the scan runs a second round
    n = len(big.g.frame)
    up, down = ulm.last_bytes()
    assert up == 64 + 4 * ((n + 15) // 16 * 16) + 4 * ((n_kfs + 15) // 16 * 16)      # the header's formula
    assert down == 4 * (len(local) + n + 2)


@pytest.mark.parametrize("n", FRAME_NS)
def test_frame_sizes(ulm, big, n):
    rng = np.random.default_rng(n)
    pts = big.g.points
    big.g.frame = [None if rng.random() < 0.1 else pts[int(rng.integers(len(pts)))] for _ in range(n)]
    order = _order(big, 3, n)
    _, frame_mp = _check(ulm.points([big.frame_points(order)])[0], big.g, order)
    if n >= 63:
        assert (frame_mp >= 0).any() and (frame_mp < 0).any()


def test_degenerate_calls(capi, ulm, big):
    g = big.g
    g.frame = g.frame[:65]
    res = ulm.points([big.frame_points([])])[0]                                      # n_kfs = 0: every live frame point is outside
    _check(res, g, [])
    assert res["n_local"] == 0 and res["n_outside"] > 0
    empty = [kf for kf in g.kfs if len(kf.matches) == 0][:2]
    assert empty
    _check(ulm.points([big.frame_points(empty)])[0], g, empty)                       # rows of length 0
    assert ulm.points([]) == []


def test_first_met_in_the_last_keyframe_and_repeats(capi, ulm, big):
    g = big.g
    order = _order(big, 3, 5)
    last = order[-1]
    rows = [lms.row_matches(kf) for kf in order]
    bad = g.bad_table()
    earlier = np.concatenate(rows[:-1])
    only_last = [s for s in rows[-1] if s >= 0 and not bad[s] and s not in earlier]
    assert only_last, "a point first met in the last named keyframe"
    flat = np.concatenate(rows)
    live = flat[(flat >= 0)]
    live = live[~bad[live]]
    uniq, counts = np.unique(live, return_counts=True)
    assert (counts >= 2).any(), "repeats across or inside rows"
    assert any((np.unique(r[r >= 0], return_counts=True)[1] >= 2).any() for r in rows if (r >= 0).any()), "a repeat inside one row"
    res = ulm.points([big.frame_points(order)])[0]
    local, _ = _check(res, g, order)
    # the first occurrence, asserted on the input: local_slot is the flat list's live entries in order of first appearance
    first = [int(np.flatnonzero(flat == s)[0]) for s in res["local_slot"]]
    assert first == sorted(first) and len(set(res["local_slot"].tolist())) == len(res["local_slot"]) == len(uniq)
    assert only_last[0] in res["local_slot"][-len(set(only_last)):]


def test_local_cap_one_below_the_count(capi, ulm, big):
    order = _order(big, 81, 7)
    full = ulm.points([big.frame_points(order)])[0]
    n = full["n_local"]
    with pytest.raises(capi.DvmError) as e:
        ulm.points([big.frame_points(order)], local_cap=n - 1)
    assert e.value.code == CAPACITY_ERR and "frame 0" in str(e.value)
    res = ulm.points([big.frame_points(order)], local_cap=n - 1, raise_capacity=False)[0]
    assert res["capacity"] and res["n_local"] == n
    _check(res, big.g, order, local_cap=n - 1)                                       # nothing past local_cap, frame_mp complete
    again = ulm.points([big.frame_points(order)])[0]                                 # idle tables behind the DVM_ERR_CAPACITY call
    assert np.array_equal(again["local_slot"], full["local_slot"]) and np.array_equal(again["frame_mp"], full["frame_mp"])
    exact = ulm.points([big.frame_points(order)], local_cap=n)[0]
    assert not exact["capacity"] and np.array_equal(exact["local_slot"], full["local_slot"])
    assert ulm.points([big.frame_points(order)], local_cap=0, raise_capacity=False)[0]["n_local"] == n


def test_batch_of_three_store_pairs(ulm, big, others):
    ps = [big, others[0], others[1]]
    orders = [_order(big, 129, 1), _order(others[0], 9, 2), _order(others[1], 3, 3)]
    single = [ulm.points([p.frame_points(o)])[0] for p, o in zip(ps, orders)]
    batch = ulm.points([p.frame_points(o) for p, o in zip(ps, orders)])
    for p, o, s, b in zip(ps, orders, single, batch):
        _check(b, p.g, o)
        for k in ("local_slot", "frame_mp"):
            assert np.array_equal(s[k], b[k])
    # one store pair in two frames of one call, with different keyframes named
    two = ulm.points([big.frame_points(orders[0]), big.frame_points(orders[0][:5])])
    _check(two[0], big.g, orders[0]); _check(two[1], big.g, orders[0][:5])


def test_ordering_behind_writes(capi, ulm, others):
    """A map-store update that sets bad, a second one that revives points, and a MATCHES patch, each followed by the call with nothing
    synchronised between."""
    p = others[1]
    g = p.g
    order = _order(p, 30, 4)
    before = ulm.points([p.frame_points(order)])[0]
    local, _ = _check(before, g, order)
    by_slot = {q.slot: q for q in g.points}
    flip = [by_slot[int(s)] for s in local[:25]]
    for q in flip:
        q.bad = True
    rec = np.zeros(len(flip), capi.LOCAL_POINT_DTYPE); rec["bad"] = 1
    p.points.update([q.slot for q in flip], rec)
    after = ulm.points([p.frame_points(order)])[0]
    _check(after, g, order)
    assert after["n_local"] == before["n_local"] - 25
    for q in flip[:10]:
        q.bad = False
    p.points.update([q.slot for q in flip[:10]], np.zeros(10, capi.LOCAL_POINT_DTYPE))
    _check(ulm.points([p.frame_points(order)])[0], g, order)
    # ReplaceMapPointMatch / EraseMapPointMatch / AddMapPoint as MATCHES edits
    kf = next(k for k in order if len(k.matches) >= 64)
    fresh = next(q for q in g.points if not q.bad and q.slot not in set(local.tolist()))
    kf.matches[0] = fresh; kf.matches[63] = None; kf.matches[1] = fresh
    p.kfs.patch_rows(capi.KFS_ROW_MATCHES, p.points, [(kf.slot, 0, fresh.slot), (kf.slot, 63, -1), (kf.slot, 1, fresh.slot)])
    res = ulm.points([p.frame_points(order)])[0]
    _check(res, g, order)
    assert fresh.slot in res["local_slot"]


def test_ordering_behind_a_commit_and_a_refresh(capi):
    """On the stores of a local-BA window (tests/ba_resident_scene.py): an update that sets bad -> BaResident.optimize -> commit -> the
    call, and MapStore.refresh that brings a new point into the store -> a MATCHES patch that names it -> the call; nothing is
    synchronised by the test between a write and the call behind it."""
    import ba_resident_scene as brs
    n_obs = np.array([1, 2, 7, 3, 4, 5, 7, 2] * 3 + [0, 0])
    w = brs.make_window(5, 8, len(n_obs), int(n_obs.sum()), 3, n_obs=n_obs, noise=0.3, iterations=10)
    pl = brs.Placed([w])
    kf_slots, mp_slots = pl.kf_slots[0], pl.mp_slots[0]
    points = [lms.MapPoint(int(s)) for s in mp_slots]
    kfs = [lms.KeyFrame(int(s), len(kf["kps"])) for s, kf in zip(kf_slots, w["kfs"])]
    for o in w["obs"]:
        kfs[o["pose"]].matches[o["kp"]] = points[o["point"]]
        points[o["point"]].add_observation(kfs[o["pose"]], int(o["kp"]))
    g = lms.Graph(kfs, points, list(points), pl.map_store.capacity, pl.kf_store.capacity, pl.kf_store.slot_keypoints)
    sl = [kf.slot for kf in kfs]
    pl.kf_store.set_rows(capi.KFS_ROW_MATCHES, pl.map_store, sl, [lms.row_matches(kf) for kf in kfs])
    u = capi.UpdateLocalMap()
    u.reserve(1, 64, len(kfs), g.map_capacity, g.kf_capacity, g.slot_keypoints)

    def call():
        order = kfs[::-1]
        res = u.points([dict(kfs=pl.kf_store, points=pl.map_store, kf_slot=[kf.slot for kf in order], mp_slot=g.frame_slots())])[0]
        return _check(res, g, order)[0]
    first = call()
    # update (bad) -> optimize -> commit -> the call: the commit writes geometry into the records the call reads `bad` from
    before = pl.map_store.read(mp_slots)
    rec = before[[2, 3, 10]].copy(); rec["bad"] = 1
    for l in (2, 3, 10):
        points[l].bad = True
    pl.map_store.update(mp_slots[[2, 3, 10]], rec)
    h = capi.BaResident()
    h.optimize(pl.problems())
    h.commit()
    after_commit = call()
    assert len(after_commit) == len(first) - 3
    now = pl.map_store.read(mp_slots)
    assert (now["pos"] != before["pos"]).any(axis=1).sum() >= 10 and list(np.flatnonzero(now["bad"])) == [2, 3, 10]      # the commit ran, bad kept
    # refresh (a new point enters the store) -> patch (two keyframes hold it) -> the call
    new_slot = int(np.setdiff1d(np.arange(g.map_capacity), mp_slots)[0])
    where = [(0, 0), (4, len(kfs[4].matches) - 1)]                                   # (keyframe, keypoint) of its two observations
    obs = np.zeros(2, capi.MP_OBS_DTYPE); obs["kf"] = [0, 1]; obs["kp"] = [kp for _, kp in where]
    kt = np.zeros(2, capi.MP_REFRESH_KF_DTYPE); kt["slot"] = [kfs[k].slot for k, _ in where]; kt["ow"] = [[0, 0, 0], [1, 0, 0]]
    pl.map_store.refresh(pl.kf_store, np.array([new_slot], np.int32), np.array([0, 2], np.int32), obs, np.zeros(1, np.int32), kt,
                         is_new=np.ones(1, np.uint8), new_pos=np.array([[0.5, 0.2, 7.0]], np.float32))
    fresh = lms.MapPoint(new_slot)
    g.points.append(fresh); g.frame.append(fresh)
    for k, kp in where:
        kfs[k].matches[kp] = fresh
    pl.kf_store.patch_rows(capi.KFS_ROW_MATCHES, pl.map_store, [(kfs[k].slot, kp, new_slot) for k, kp in where])
    after_refresh = call()
    assert new_slot in after_refresh and new_slot not in after_commit
    # refresh of OLD points (descriptor and geometry rewritten in place, bad kept) -> the call
    old = np.array([0, 1], np.int32)
    oo = w["obs"][np.isin(w["obs"]["point"], old)]
    order_ = np.argsort(oo["point"], kind="stable")
    oo = oo[order_]
    obs2 = np.zeros(len(oo), capi.MP_OBS_DTYPE); obs2["kf"] = oo["pose"]; obs2["kp"] = oo["kp"]
    kt2 = np.zeros(len(kfs), capi.MP_REFRESH_KF_DTYPE); kt2["slot"] = sl
    off = np.r_[0, np.cumsum(np.bincount(oo["point"], minlength=2)[:2])].astype(np.int32)
    pl.map_store.refresh(pl.kf_store, mp_slots[old], off, obs2, np.zeros(2, np.int32), kt2)
    assert np.array_equal(call(), after_refresh)
    u.close(); h.close()
    pl.kf_store.close(); pl.map_store.close()


def test_refusals(capi, ulm, big, others):
    order = _order(big, 3, 9)
    ok = big.frame_points(order)
    want = ulm.points([ok])[0]
    free = next(s for s in range(KF_CAPACITY) if s not in {kf.slot for kf in big.g.kfs})
    unwritten = next(s for s in range(MAP_CAPACITY) if s not in {x.slot for x in big.g.points})
    sl = [kf.slot for kf in order]
    rowless = lms.Placed(capi, big.g, rows=False)
    cases = [
        ("frame slot below -1", [dict(ok, mp_slot=np.array([3, -2], np.int32))], INVALID, "frame 0, entry 1 (slot -2)"),
        ("frame slot never written", [ok, dict(ok, mp_slot=np.array([unwritten], np.int32))], INVALID, "frame 1, entry 0 (slot %d)" % unwritten),
        ("frame slot outside", [dict(ok, mp_slot=np.array([MAP_CAPACITY], np.int32))], INVALID, "frame 0, entry 0"),
        ("kf_slot outside", [dict(ok, kf_slot=sl + [KF_CAPACITY])], INVALID, "entry 3 (slot %d): kf_slot outside" % KF_CAPACITY),
        ("kf_slot negative", [dict(ok, kf_slot=sl + [-1])], INVALID, "entry 3 (slot -1): kf_slot outside"),
        ("kf_slot never put", [dict(ok, kf_slot=[free])], INVALID, "entry 0 (slot %d): kf_slot outside" % free),
        ("kf_slot without a row", [dict(kfs=rowless.kfs, points=rowless.points, mp_slot=ok["mp_slot"], kf_slot=sl)], INVALID, "without a MATCHES row"),
        ("kf_slot twice", [dict(ok, kf_slot=sl + [sl[0]])], INVALID, "entry 3 (slot %d): kf_slot named twice" % sl[0]),
        ("row of another map", [dict(ok, points=others[0].points, mp_slot=np.zeros(0, np.int32))], INVALID, "another map store"),
        ("too many frames", [ok] * 4, CAPACITY_ERR, "max_frames"),
        ("too many keypoints", [dict(ok, mp_slot=np.full(1026, -1, np.int32))], CAPACITY_ERR, "max_frame_keypoints"),
        ("too many keyframes", [dict(ok, kf_slot=[kf.slot for kf in big.g.kfs])], CAPACITY_ERR, "max_local_keyframes"),
    ]
    for name, frames, code, text in cases:
        with pytest.raises(capi.DvmError) as e:
            ulm.points(frames)
        assert e.value.code == code and text in str(e.value), (name, str(e.value))
        got = ulm.points([ok])[0]                                                    # the handle stays usable, its tables idle
        assert np.array_equal(got["local_slot"], want["local_slot"]) and np.array_equal(got["frame_mp"], want["frame_mp"])
    rowless.close()
    fresh = capi.UpdateLocalMap()
    with pytest.raises(capi.DvmError) as e:
        fresh.points([ok])
    assert e.value.code == CAPACITY_ERR
    fresh.close()
