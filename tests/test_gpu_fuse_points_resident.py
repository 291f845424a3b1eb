"""dvm_fuse_targets_run[_hits]_resident: the Fuse run on points named as slots of a dvm_map_store.  Every comparison is array_equal against
dvm_fuse_targets_run / _run_hits on the table built from MapStore.read of the same slots (fuse_points_scene.table): the scenes of
tests/test_gpu_fuse_resident.py on uploaded and on resident targets, lane and block tails of the gather, the masks (a slot of -1, a slot
twice, a bad record, valid, skip), the ordering against update / refresh / a local BA's commit with nothing synchronised in between,
every refusal followed by a good call, and the byte counter."""
import numpy as np
import pytest

import ba_resident_scene as brs
import fuse_cam_scene as fcs
import fuse_points_scene as fps
import fuse_targets_scene as fts
import map_refresh_scene as mrs
import test_gpu_fuse_resident as tfr

pytestmark = pytest.mark.gpu

N_PTS = tfr.N_PTS
MAX_PTS = 300
STATE, INVALID, CAPACITY = -6, -1, -3


def gap_slots(n, top):
    """n slots descending from top with gaps of 2 and 3"""
    s = top - np.cumsum(np.r_[0, 2 + (np.arange(max(n - 1, 0)) % 2)])[:n]
    assert n == 0 or s.min() >= 0
    return s.astype(np.int32)


def place(capi, pts, bad=None):
    """(store, slots): the points' records at descending slots with gaps"""
    n = len(pts["pos"])
    store = capi.MapStore(3 * n + 4)
    slots = gap_slots(n, store.capacity - 1)
    if n:
        store.update(slots, fps.records(pts, bad))
    return store, slots


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.FuseTargets()
    h.reserve(MAX_PTS, 8, 5 * 700 + tfr.SLOT_KEYPOINTS)
    h.reserve_hits(8 * MAX_PTS)
    yield h
    h.close()


@pytest.fixture(scope="module")
def resident_chain(capi):
    h = capi.FuseTargets()
    h.reserve(MAX_PTS, 8, 0)
    h.reserve_hits(8 * MAX_PTS)
    yield h
    h.close()


def uploaded(h, tab, th, skip):
    return (*h.run(tab, th, skip), *h.run_hits(tab, th, skip))


def resident(h, store, slots, th, skip, valid=None):
    return (*h.run_resident(store, slots, th, skip, valid), *h.run_hits_resident(store, slots, th, skip, valid))


def assert_same(got, want):
    for a, b, name in zip(got, want, ("best_idx", "best_dist", "hit_off", "hits")):
        assert np.array_equal(a, b), name


def check(h, store, slots, th, skip, valid=None):
    """the resident run first, the table read behind it; returns the uploaded rows without skip"""
    got = [resident(h, store, slots, th, sk, valid) for sk in (None, skip)]
    tab = fps.read_table(store, slots, valid)
    want = [uploaded(h, tab, th, sk) for sk in (None, skip)]
    for g, w in zip(got, want):
        assert_same(g, w)
    return want[0]


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("kind", ["pinhole", "scw", "robomaster", "tum", "mixed"])
def test_rows_equal_the_uploaded_call(capi, chain, resident_chain, kind, T):
    tg, models, forms, pts, skip, th = tfr._case(capi, kind, T)
    n_t = len(tg)
    store, slots = place(capi, pts)
    chain.set(tg, models=models, forms=forms)
    want = uploaded(chain, fps.read_table(store, slots, pts["valid"]), th, None)
    assert (want[0] >= 0).sum() >= (5 if kind != "mixed" else 1)
    check(chain, store, slots, th, skip, pts["valid"])
    kfs = capi.KeyframeStore(n_t, tfr.SLOT_KEYPOINTS)
    kfs.put(range(n_t), [tfr._putable(kf) for kf in tg])
    resident_chain.set_resident(kfs, range(n_t), [tfr._pose(kf) for kf in tg], models=models, forms=forms)
    assert_same(check(resident_chain, store, slots, th, skip, pts["valid"]), want)
    kfs.close(); store.close()


@pytest.fixture(scope="module")
def two_targets(chain):
    sc = fts.scene(2, 2, MAX_PTS)
    chain.set(sc["targets"])
    return sc


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_tails(capi, chain, two_targets, n):
    sc = fts.prefix(two_targets, n)
    chain.set(sc["targets"])
    store, slots = place(capi, sc["pts"])
    assert n < 3 or set(np.diff(slots)) == {-2, -3} or n == 2
    want = check(chain, store, slots, 3.0, sc["skip"], sc["pts"]["valid"])
    assert n < 63 or (want[0] >= 0).any()
    store.close()


def test_masks(capi, chain, two_targets):
    sc = fts.prefix(two_targets, N_PTS)
    chain.set(sc["targets"])
    pts, skip = sc["pts"], sc["skip"]
    base = uploaded(chain, dict(pts, valid=None), 3.0, None)
    hit = np.flatnonzero((base[0] >= 0).any(axis=0))
    assert len(hit) >= 8
    bad = np.zeros(N_PTS, np.int32); bad[hit[:3]] = 1
    store, slots = place(capi, pts, bad)
    assert (store.read(slots[hit[:3]])["bad"] == 1).all() and store.read(slots)["bad"].sum() == 3      # as constructed
    # a bad record masks its row with no valid given; skip given and absent (check runs both)
    rows = check(chain, store, slots, 3.0, skip)
    assert (rows[0][:, hit[:3]] == -1).all() and (rows[1][:, hit[:3]] == 256).all() and (rows[0][:, hit[3:]] >= 0).any()
    # valid given
    rows_v = check(chain, store, slots, 3.0, skip, pts["valid"])
    assert not np.array_equal(rows_v[0], rows[0]) and (rows_v[0][:, pts["valid"] == 0] == -1).all()
    # a slot of -1, a slot named twice
    s2 = slots.copy(); s2[hit[4]] = -1; s2[hit[5]] = s2[hit[6]]
    rows2 = check(chain, store, s2, 3.0, skip)
    assert (rows2[0][:, hit[4]] == -1).all() and np.array_equal(rows2[0][:, hit[5]], rows2[0][:, hit[6]]) and np.array_equal(rows2[1][:, hit[5]], rows2[1][:, hit[6]])
    assert (rows2[0][:, hit[6]] >= 0).any()
    # all rows masked: three ways
    for sl, va, st in ((np.full(N_PTS, -1, np.int32), None, store), (np.full(N_PTS, -1, np.int32), None, None), (slots, np.zeros(N_PTS, np.uint8), store)):
        bi, bd, off, hits = resident(chain, st, sl, 3.0, None, va)
        assert (bi == -1).all() and (bd == 256).all() and (off == 0).all() and len(hits) == 0
    # n = 0
    bi, bd, off, hits = resident(chain, store, np.zeros(0, np.int32), 3.0, None)
    assert bi.shape == (2, 0) and (off == 0).all() and len(hits) == 0
    store.close()


def test_ordering_against_update(capi, chain, two_targets):
    """update -> run_resident; run_resident -> update -> run_resident: nothing synchronised in between"""
    sc = fts.prefix(two_targets, N_PTS)
    chain.set(sc["targets"])
    pts = sc["pts"]
    store = capi.MapStore(3 * N_PTS + 4)
    slots = gap_slots(N_PTS, store.capacity - 1)
    recs = fps.records(pts)
    store.update(slots, recs)                                                # update -> run
    first = resident(chain, store, slots, 3.0, None)
    assert_same(first, uploaded(chain, fps.table(recs, slots), 3.0, None))
    hit = np.flatnonzero((first[0] >= 0).any(axis=0))
    assert len(hit) >= 5
    moved = recs.copy()
    moved["desc"][hit] ^= np.uint8(0xFF)                                     # another descriptor on rows that had hits
    store.update(slots[hit], moved[hit])                                     # run -> update -> run
    second = resident(chain, store, slots, 3.0, None)
    assert_same(second, uploaded(chain, fps.table(moved, slots), 3.0, None))
    assert not np.array_equal(second[0], first[0]) and (second[0][:, hit] == -1).all()
    assert store.read(slots).tobytes() == moved.tobytes()
    store.close()


def test_ordering_behind_a_refresh(capi, chain, two_targets):
    """MapStore.refresh(DESCRIPTOR) -> run_resident: the stale-descriptor re-run names slots only"""
    sc = fts.prefix(two_targets, N_PTS)
    chain.set(sc["targets"])
    base = uploaded(chain, dict(sc["pts"], valid=None), 3.0, None)
    hit = np.flatnonzero((base[0] >= 0).any(axis=0))[:20]
    counts = np.zeros(N_PTS, int); counts[hit] = 3
    kfs = [mrs.make_keyframe(40 + k, 200) for k in range(6)]
    rs = mrs.make_scene(31, kfs, list(counts), distinct=False)
    store, slots = place(capi, sc["pts"])
    kf_store = capi.KeyframeStore(6, 256)
    kf_store.put(range(6), kfs)
    args, kw = mrs.call_args(rs, slots, np.arange(6, dtype=np.int32))
    out = store.refresh(kf_store, *args, what=mrs.DESCRIPTOR, **kw)
    got = resident(chain, store, slots, 3.0, None)
    after = store.read(slots)
    assert (out["best_obs"][hit] >= 0).all() and (after["desc"][hit] != sc["pts"]["desc"][hit]).any(axis=1).all()
    assert_same(got, uploaded(chain, fps.table(after, slots), 3.0, None))
    assert not np.array_equal(got[0], base[0])
    stale = slots[hit]                                                       # the re-run of the stale slots alone
    assert_same(resident(chain, store, stale, 3.0, None), uploaded(chain, fps.table(after[hit], stale), 3.0, None))
    kf_store.close(); store.close()


def test_ordering_behind_a_local_ba_commit(capi, chain, two_targets):
    """BaResident.optimize -> commit -> run_resident: the positions are the committed ones"""
    chain.set(two_targets["targets"])
    n_obs = np.array([1, 2, 7, 3, 4, 5, 7, 2] * 3 + [0, 0])
    w = brs.make_window(5, 8, len(n_obs), int(n_obs.sum()), 3, n_obs=n_obs, noise=0.3, iterations=10)
    pl = brs.Placed([w])
    slots = pl.mp_slots[0]
    before = pl.map_store.read(slots)
    h = capi.BaResident()
    h.optimize(pl.problems())
    h.commit()
    got = resident(chain, pl.map_store, slots, 3.0, None)
    after = pl.map_store.read(slots)
    assert (after["pos"] != before["pos"]).any(axis=1).sum() >= 10
    assert_same(got, uploaded(chain, fps.table(after, slots), 3.0, None))
    h.close()
    for s in (pl.kf_store, pl.map_store):
        s.close()


def test_a_put_to_a_named_keyframe_slot(capi, resident_chain):
    tg, _, _, pts, skip, th = tfr._case(capi, "pinhole", 5)
    kfs = capi.KeyframeStore(5, tfr.SLOT_KEYPOINTS)
    kfs.put(range(5), [tfr._putable(kf) for kf in tg])
    store, slots = place(capi, pts)
    h = resident_chain
    h.set_resident(kfs, range(5), [tfr._pose(kf) for kf in tg])
    want = check(h, store, slots, th, skip)
    kfs.put([3], [tfr._putable(tg[3])])
    for run in (lambda: h.run_resident(store, slots, th, skip), lambda: h.run_hits_resident(store, slots, th, skip)):
        with pytest.raises(capi.DvmError) as e:
            run()
        assert e.value.code == STATE and "a target's slot was written since the set" in str(e.value)
    h.set_resident(kfs, range(5), [tfr._pose(kf) for kf in tg])
    assert_same(resident(h, store, slots, th, None), want)
    kfs.close(); store.close()


def test_refusals_each_followed_by_a_good_call(capi, chain, two_targets):
    sc = fts.prefix(two_targets, N_PTS)
    chain.set(sc["targets"])
    store, slots = place(capi, sc["pts"])
    want = check(chain, store, slots, 3.0, sc["skip"])
    unwritten = int(slots[0]) - 1
    assert unwritten not in set(slots.tolist())
    big = np.concatenate([slots, slots])[:MAX_PTS + 1]
    cases = ((store, [store.capacity], INVALID), (store, [unwritten], INVALID), (store, [-2], INVALID), (None, [int(slots[0])], INVALID), (store, big, CAPACITY))
    for st, bad_slots, code in cases:
        sl = slots.copy() if len(bad_slots) == 1 else np.asarray(bad_slots, np.int32)
        if len(bad_slots) == 1:
            sl[7] = bad_slots[0]
        out = (np.full((2, len(sl)), -9, np.int32), np.full((2, len(sl)), -9, np.int32))
        with pytest.raises(capi.DvmError) as e:
            chain.run_resident(st, sl, 3.0, out=out)
        assert e.value.code == code, (bad_slots[:1], str(e.value))
        assert (out[0] == -9).all() and (out[1] == -9).all()
        with pytest.raises(capi.DvmError) as e:
            chain.run_hits_resident(st, sl, 3.0)
        assert e.value.code == code and (e.value.hit_off == -7).all() and e.value.n_hits == -7
        assert_same(resident(chain, store, slots, 3.0, None), want)
    fresh = capi.FuseTargets()                                               # run before set
    fresh.reserve(MAX_PTS, 2, 0); fresh.reserve_hits(16)
    out = (np.full((0, N_PTS), -9, np.int32), np.full((0, N_PTS), -9, np.int32))
    with pytest.raises(capi.DvmError) as e:
        fresh.run_resident(store, slots, 3.0, out=out)
    assert e.value.code == INVALID and "no targets" in str(e.value)
    with pytest.raises(capi.DvmError) as e:
        fresh.run_hits_resident(store, slots, 3.0)
    assert e.value.code == INVALID
    fresh.close()
    assert_same(resident(chain, store, slots, 3.0, None), want)
    store.close()


def test_byte_counter(capi, chain, two_targets):
    pad = lambda b: (b + 63) // 64 * 64                                      # noqa: E731
    T = 2
    for n in (65, N_PTS):
        sc = fts.prefix(two_targets, n)
        chain.set(sc["targets"])
        store, slots = place(capi, sc["pts"])
        for valid, skip in ((None, None), (sc["pts"]["valid"], None), (None, sc["skip"]), (sc["pts"]["valid"], sc["skip"])):
            want = pad(4 * n) + (pad(n) if valid is not None else 0) + (pad(T * n) if skip is not None else 0)
            chain.run_resident(store, slots, 3.0, skip, valid)
            assert chain.last_upload_bytes()[1] == want
            chain.run_hits_resident(store, slots, 3.0, skip, valid)
            assert chain.last_upload_bytes()[1] == want
        chain.run(fps.read_table(store, slots), 3.0, sc["skip"])
        assert chain.last_upload_bytes()[1] > 65 * n                         # the uploaded table, for scale
        store.close()
