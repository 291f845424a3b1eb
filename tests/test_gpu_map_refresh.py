"""dvm_map_store_refresh (capi.MapStore.refresh): every record, best_obs, best_median and geometry row is compared bit for bit with the
path an integrator has without the call -- gather the rows, capi.distinctive_descriptors, the numpy restatement's record
(map_refresh_scene.refresh_ref), MapStore.update on a SECOND store, read.  Sizes around the wave and up to the 512 limit, ties, bad
keyframes with and without a slot, the ref observation's place, two level tables, what = one group only, new points, the ordering
against update / put / a local BA's commit, every refusal followed by a good call, and what travels."""
import ctypes as C

import numpy as np
import pytest

import ba_resident_scene as brs
import map_refresh_scene as S

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID, CAPACITY_ERR = -1, -3


def gap_slots(n, top):
    """n slots descending from top with gaps of 2 and 3"""
    s = top - np.cumsum(np.r_[0, 2 + (np.arange(max(n - 1, 0)) % 2)])[:n]
    assert n == 0 or s.min() >= 0
    return s.astype(np.int32)


class Placed:
    """The scene's keyframes in a KeyframeStore, its OLD points' records in two MapStores (a: refreshed, b: today's path), slots descending
    with gaps of 2 and 3; the new points' slots are not written."""

    def __init__(self, sc, put=True):
        from dvm_slam_amd import capi
        self.sc = sc
        K, n = len(sc["kfs"]), len(sc["records"])
        self.kf_store = capi.KeyframeStore(3 * K + 4, max(max(len(k["kps"]) for k in sc["kfs"]), 64))
        self.a, self.b = capi.MapStore(3 * n + 4), capi.MapStore(3 * n + 4)
        self.kf_slots, self.mp_slots = gap_slots(K, self.kf_store.capacity - 1), gap_slots(n, self.a.capacity - 1)
        self.old = sc["is_new"] == 0
        if self.old.any():
            self.a.update(self.mp_slots[self.old], sc["records"][self.old]); self.b.update(self.mp_slots[self.old], sc["records"][self.old])
        if put:
            live = ~sc["gone"]
            self.kf_store.put(self.kf_slots[live], [kf for kf, l in zip(sc["kfs"], live) if l])

    def refresh(self, what=S.BOTH, want_geometry=True, store=None):
        args, kw = S.call_args(self.sc, self.mp_slots, self.kf_slots)
        return (store or self.a).refresh(self.kf_store, *args, what=what, want_geometry=want_geometry, **kw)

    def close(self):
        for h in (self.a, self.b, self.kf_store):
            h.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def check(sc, what=S.BOTH, pl=None):
    """refresh on store a, today's path on store b: outputs and records bit-equal.  Returns (placed, out, records)."""
    pl = pl or Placed(sc)
    before = np.zeros(len(sc["records"]), sc["records"].dtype)
    if pl.old.any():
        before[pl.old] = pl.a.read(pl.mp_slots[pl.old])
    out = pl.refresh(what)
    rec, best, med, geo = S.host_path(sc, pl.b, pl.mp_slots, what, before=before)
    assert np.array_equal(out["best_obs"], best), np.flatnonzero(out["best_obs"] != best)
    assert np.array_equal(out["best_median"], med), np.flatnonzero(out["best_median"] != med)
    assert out["geometry"].tobytes() == geo.tobytes(), np.flatnonzero((bits(out["geometry"]) != bits(geo)).reshape(len(geo), -1).any(axis=1))
    got, want = pl.a.read(pl.mp_slots), pl.b.read(pl.mp_slots)
    assert want.tobytes() == rec.tobytes()
    assert got.tobytes() == want.tobytes(), np.flatnonzero((bits(got) != bits(want)).reshape(len(got), -1).any(axis=1))
    return pl, out, rec


def keyframes(n_kf, n_kp, seed=0):
    return [S.make_keyframe(seed + k, n_kp + 7 * k, S.TABLES_B if k % 2 else S.TABLES_A) for k in range(n_kf)]


@pytest.fixture(scope="module")
def kfs12():
    return keyframes(12, 300)


def test_sizes_around_the_wave_and_the_limit(kfs12):
    """N = 1, 2, 3, 63, 64, 65, 512 beside points without observations; both level tables; ref keypoints at octave 0 and n_levels - 1; kp = 0
    and n - 1"""
    counts = [1, 0, 2, 3, 63, 0, 64, 65, 512, 0, 7, 200]
    sc = S.make_scene(2, [dict(kf, kps=kf["kps"].copy()) for kf in kfs12], counts, distinct=False)      # (octaves are set below: its own copy)
    o, off = sc["obs"], sc["obs_off"]
    for p, octave_of in ((4, lambda nl: 0), (6, lambda nl: nl - 1), (7, lambda nl: 0), (8, lambda nl: nl - 1)):
        r = o[off[p] + sc["ref_obs"][p]]
        kf = sc["kfs"][r["kf"]]
        kf["kps"]["octave"][r["kp"]] = octave_of(len(kf["scale_factors"]))
    tables = {len(sc["kfs"][o[off[p] + sc["ref_obs"][p]]["kf"]]["scale_factors"]) for p in range(len(counts)) if counts[p]}
    assert tables == {5, 8}
    assert (o["kp"] == 0).any() and any(o["kp"][j] == len(sc["kfs"][o["kf"][j]]["kps"]) - 1 for j in range(len(o)))
    pl, out, rec = check(sc)
    assert np.array_equal(rec["n_obs"], counts) and (out["best_obs"][np.array(counts) == 0] == -1).all() and (out["best_obs"][np.array(counts) > 0] >= 0).all()
    pl.close()


def test_full_wave_in_the_form_without_lds(kfs12):
    """no list beyond 64: the call takes the kernel form without LDS, with a list that fills the wave and bad keyframes inside it"""
    sc = S.make_scene(3, kfs12, [64, 63, 0, 1, 33], bad=[2, 5], distinct=False)
    assert sc["bad"][sc["obs"]["kf"][:64]].any() and not sc["bad"][sc["obs"]["kf"][:64]].all()
    check(sc)[0].close()


def test_ties_on_one_keyframe():
    """n_kfs = 1; all rows identical (winner 0); two equal medians, the first wins; a set whose winner is the LAST row"""
    kf = S.make_keyframe(3, 64)
    d = np.zeros((12, 32), np.uint8)

    def row(*bit_ranges):
        b = np.zeros(256, np.uint8)
        for lo, hi in bit_ranges:
            b[lo:hi] = 1
        return np.packbits(b)
    d[0:4] = row((5, 50))                                                  # point 0: four identical rows
    d[4], d[5], d[6] = row(), row((0, 4)), row((8, 16))                     # point 1: medians 4, 4, 8
    d[7], d[8], d[9], d[10], d[11] = row((0, 10)), row((20, 30)), row((40, 50)), row((60, 70)), row()   # point 2: medians 20 x 4, then 10
    kf["desc"][:12] = d
    sc = S.make_scene(4, [kf], [4, 3, 5], kp_of={0: [0, 1, 2, 3], 1: [4, 5, 6], 2: [7, 8, 9, 10, 11]})
    med = [np.sort(S.hamming_table(S.rows_of(sc, p)[0]), axis=1)[:, (n - 1) >> 1].tolist() for p, n in enumerate([4, 3, 5])]
    assert med == [[0, 0, 0, 0], [4, 4, 8], [20, 20, 20, 20, 10]]           # as constructed
    pl, out, rec = check(sc)
    assert out["best_obs"].tolist() == [0, 0, 4] and out["best_median"].tolist() == [0, 4, 10]
    assert len(pl.kf_slots) == 1 and np.array_equal(np.diff(pl.mp_slots), [-2, -3])
    pl.close()


def test_bad_keyframes(kfs12):
    """an observation on a bad keyframe leaves the candidates (the winner moves) and stays in the normal and in n_obs; all observations bad:
    best_obs = -1, the descriptor bytes as before, the geometry written; a bad entry with slot = -1"""
    counts = [5, 6, 4, 3, 9]
    free = S.make_scene(7, kfs12, counts)
    w_all = S.distinctive(S.rows_of(free, 0, candidates_only=False)[0])[0]
    bad_kf = int(free["obs"]["kf"][w_all])                                  # the keyframe that holds point 0's winner
    others = [k for k in range(12) if k != bad_kf][:3]
    sc = S.make_scene(7, kfs12, counts, bad=[bad_kf, others[0], others[1]], gone=[others[1]],
                      kf_of={2: [bad_kf, others[0], bad_kf, others[0]], 3: [others[1], others[2], others[1]]})
    assert np.array_equal(sc["obs"][:5], free["obs"][:5])
    pl, out, rec = check(sc)
    assert out["best_obs"][0] not in (-1, w_all) and rec["n_obs"][0] == 5
    g_all = S.geometry(sc["records"]["pos"][0], sc["ow"][sc["obs"]["kf"][:5]], sc["ow"][sc["obs"]["kf"][sc["ref_obs"][0]]], np.ones(8, F32), 0)
    assert np.array_equal(rec["normal"][0], g_all[3:6])                     # all five terms, the bad keyframe's too
    assert out["best_obs"][2] == -1 and out["best_median"][2] == -1 and np.array_equal(rec["desc"][2], sc["records"]["desc"][2])
    assert not np.array_equal(rec["normal"][2], sc["records"]["normal"][2]) and rec["n_obs"][2] == 4
    assert sc["gone"][sc["obs"]["kf"][sc["obs_off"][3]]] and out["best_obs"][3] == 1       # the one observation on a keyframe that is not bad
    pl.close()


@pytest.mark.parametrize("ref", ["first", "mid", "last"])
def test_ref_observation_place(kfs12, ref):
    sc = S.make_scene(11, kfs12, [1, 4, 9, 12, 2], ref=ref)
    want = {"first": 0, "mid": None, "last": -1}[ref]
    if want is not None:
        assert all(sc["ref_obs"][p] == (0 if want == 0 else n - 1) for p, n in enumerate([1, 4, 9, 12, 2]))
    else:
        assert 0 < sc["ref_obs"][3] < 11
    check(sc)[0].close()


def test_one_group_only(kfs12):
    sc = S.make_scene(13, kfs12, [3, 0, 8, 70, 2], distinct=False)
    pl, out, rec = check(sc, S.DESCRIPTOR)
    before = sc["records"]
    for f in ("pos", "normal", "min_dist", "max_dist", "bad"):
        assert rec[f].tobytes() == before[f].tobytes(), f
    assert (rec["desc"][[0, 2, 3, 4]] != before["desc"][[0, 2, 3, 4]]).any(axis=1).all() and np.array_equal(rec["n_obs"], [3, 0, 8, 70, 2])
    assert out["geometry"].tobytes() == np.column_stack([before["pos"], before["normal"], before["min_dist"], before["max_dist"]]).astype(F32).tobytes()
    pl.close()
    pl, out, rec = check(sc, S.GEOMETRY)
    assert rec["desc"].tobytes() == before["desc"].tobytes() and rec["pos"].tobytes() == before["pos"].tobytes() and (out["best_obs"] == -1).all()
    assert (rec["normal"][[0, 2, 3, 4]] != before["normal"][[0, 2, 3, 4]]).any(axis=1).all() and np.array_equal(rec["normal"][1], before["normal"][1])
    pl.close()


@pytest.mark.parametrize("new", [[0, 1, 2, 3], [1, 3]])
def test_new_points(kfs12, new):
    """a call of new points only and a mixed one: the slot cannot be read before, holds the restatement's 72 bytes with bad = 0 after, and
    is a written slot from then on; old points keep pos and bad (records with bad = 1 among them)"""
    from dvm_slam_amd import capi
    sc = S.make_scene(17, kfs12, [2, 2, 5, 66], new=new, distinct=False)
    sc["records"]["bad"][[0, 2]] = 1
    pl = Placed(sc)
    for p in new:
        with pytest.raises(capi.DvmError) as ei:
            pl.a.read(pl.mp_slots[p:p + 1])
        assert ei.value.code == INVALID
    _, out, rec = check(sc, pl=pl)
    assert (rec["bad"][new] == 0).all() and np.array_equal(rec["pos"][new], sc["new_pos"][new]) and (out["best_obs"][new] >= 0).all()
    old = [p for p in range(4) if p not in new]
    assert np.array_equal(rec["pos"][old], sc["records"]["pos"][old]) and np.array_equal(rec["bad"][old], sc["records"]["bad"][old])
    assert len(old) == 0 or rec["bad"][old].max() == 1
    again = pl.a.read(pl.mp_slots[new])                                     # accepted now
    assert again.tobytes() == rec[new].tobytes()
    pl.close()


def test_ordering_against_update_and_put(kfs12):
    """update -> refresh -> read; refresh -> update -> read; KeyframeStore.put -> refresh; two refreshes back to back: nothing synchronised
    in between"""
    sc = S.make_scene(19, kfs12, [4, 6, 3, 65, 1], distinct=False)
    pl = Placed(sc, put=False)
    moved = sc["records"].copy()
    moved["pos"] += F32(0.25); moved["desc"] ^= np.uint8(0x5A)
    sc2 = dict(sc, records=moved)
    pl.kf_store.put(pl.kf_slots, sc["kfs"])                                 # put -> refresh
    pl.a.update(pl.mp_slots, moved)                                         # update -> refresh -> read
    out = pl.refresh()
    got = pl.a.read(pl.mp_slots)
    rec, best, med, geo = S.refresh_ref(sc2)
    assert got.tobytes() == rec.tobytes() and np.array_equal(out["best_obs"], best) and out["geometry"].tobytes() == geo.tobytes()
    out = pl.refresh()                                                      # refresh -> update -> read
    pl.a.update(pl.mp_slots[:2], sc["records"][:2])
    got = pl.a.read(pl.mp_slots)
    assert got[:2].tobytes() == sc["records"][:2].tobytes() and got[2:].tobytes() == rec[2:].tobytes()
    a = pl.refresh(S.GEOMETRY); b = pl.refresh(S.DESCRIPTOR)                # two calls back to back
    rec2 = S.refresh_ref(dict(sc, records=got))[0]
    assert pl.a.read(pl.mp_slots).tobytes() == rec2.tobytes() and (a["best_obs"] == -1).all() and np.array_equal(b["best_obs"], best)
    other = [S.make_keyframe(100 + k, len(kf["kps"]), S.TABLES_B if k % 2 else S.TABLES_A) for k, kf in enumerate(sc["kfs"])]
    pl.kf_store.put(pl.kf_slots, other)                                     # refresh -> put -> refresh: the new rows
    pl.refresh()
    assert pl.a.read(pl.mp_slots).tobytes() == S.refresh_ref(dict(sc, kfs=other, records=rec2))[0].tobytes()
    pl.close()


def test_refresh_behind_a_local_ba_commit():
    """BaResident.optimize -> commit -> refresh(GEOMETRY) -> read: the normal is the one of the COMMITTED positions"""
    from dvm_slam_amd import capi
    n_obs = np.array([1, 2, 7, 3, 4, 5, 7, 2] * 3 + [0, 0])
    w = brs.make_window(5, 8, len(n_obs), int(n_obs.sum()), 3, n_obs=n_obs, noise=0.3, iterations=10)
    pl = brs.Placed([w])
    before = pl.map_store.read(pl.mp_slots[0])
    h = capi.BaResident()
    r = h.optimize(pl.problems())[0]
    h.commit()
    o = w["obs"]
    order = np.argsort(o["point"], kind="stable")                           # a point's edges ascending: the caller's order
    off = np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int32)
    obs = np.zeros(len(o), capi.MP_OBS_DTYPE); obs["kf"] = o["pose"][order]; obs["kp"] = o["kp"][order]
    ref = np.array([0 if n_obs[l] == 0 else int(np.flatnonzero(order[off[l]:off[l + 1]] == w["ref_edge"][l])[0]) for l in range(len(n_obs))], np.int32)
    kt = np.zeros(8, capi.MP_REFRESH_KF_DTYPE); kt["slot"] = pl.kf_slots[0]; kt["ow"] = r["ow"]
    out = pl.map_store.refresh(pl.kf_store, pl.mp_slots[0], off, obs, ref, kt, what=S.GEOMETRY, want_geometry=True)
    after = pl.map_store.read(pl.mp_slots[0])
    geom, dirty, centres, state = brs.prepare_ref(w, r)
    clean = state == 0
    assert clean.sum() >= 20 and (geom[clean, :3] != before["pos"][clean]).any(axis=1).all()      # the commit moved them
    assert after["pos"][clean].tobytes() == geom[clean, :3].tobytes()
    sc = dict(kfs=w["kfs"], ow=r["ow"], bad=np.zeros(8, bool), gone=np.zeros(8, bool), obs_off=off, obs=obs, ref_obs=ref, is_new=np.zeros(len(n_obs), np.uint8),
              new_pos=None, records=brs.committed_records(before, geom, state))
    rec, _, _, geo = S.refresh_ref(sc, S.GEOMETRY)
    assert after.tobytes() == rec.tobytes() and out["geometry"].tobytes() == geo.tobytes()
    assert after[clean].tobytes() == sc["records"][clean].tobytes()         # the very bits the commit wrote: one definition
    h.close()
    for s in (pl.kf_store, pl.map_store):
        s.close()


def test_no_points():
    from dvm_slam_amd import capi
    ks, ms = capi.KeyframeStore(2, 64), capi.MapStore(4)
    out = ms.refresh(ks, np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, capi.MP_OBS_DTYPE), np.zeros(0, np.int32), np.zeros(0, capi.MP_REFRESH_KF_DTYPE))
    assert len(out["best_obs"]) == 0 and ms.last_refresh_bytes() == (0, 0)
    ks.close(); ms.close()


def test_refusals_each_followed_by_a_good_call(kfs12):
    from dvm_slam_amd import capi
    counts = [3, 5, 0, 66, 4, 2]
    sc = S.make_scene(23, kfs12, counts, bad=[11], gone=[11], new=[5], distinct=False, kf_of={4: [0, 11, 1, 2]})
    n = len(counts)
    pl = Placed(sc)
    pl.kf_store.put(np.array([0, 1], np.int32), kfs12[:2]); pl.kf_store.remove(np.array([1], np.int32))      # slot 1: removed; slot 2: never written
    (slots, off, obs, ref, kt), kw = S.call_args(sc, pl.mp_slots, pl.kf_slots)
    old_slots = pl.mp_slots[:5]
    expect = S.host_path(dict(sc, is_new=np.zeros(n, np.uint8)), pl.b, pl.mp_slots, before=sc["records"])
    want_old = pl.b.read(old_slots)
    gone_at = int(np.flatnonzero(obs["kf"][off[4]:off[5]] == 11)[0])

    def refused(code, what=S.BOTH, **ch):
        a = dict(mp_slots=slots.copy(), obs_off=off.copy(), obs=obs.copy(), ref_obs=ref.copy(), kfs=kt.copy(), is_new=kw["is_new"].copy(), new_pos=kw["new_pos"].copy())
        for k, f in ch.items():
            f(a[k])
        before = pl.a.read(old_slots)
        left = dict(best_obs=np.zeros(n, np.int32), best_median=np.zeros(n, np.int32), geometry=np.zeros((n, 8), F32))
        with pytest.raises(capi.DvmError) as ei:
            pl.a.refresh(pl.kf_store, a["mp_slots"], a["obs_off"], a["obs"], a["ref_obs"], a["kfs"], is_new=a["is_new"], new_pos=a["new_pos"], what=what, out=left)
        assert ei.value.code == code and "dvm_map_store_refresh" in str(ei.value), str(ei.value)
        assert not left["best_obs"].any() and not left["best_median"].any() and not left["geometry"].any()
        assert pl.a.read(old_slots).tobytes() == before.tobytes()
        with pytest.raises(capi.DvmError):
            pl.a.read(slots[5:6])                                           # the new slot is still unwritten
        out = pl.a.refresh(pl.kf_store, slots[:5], off[:6], obs[:off[5]], ref[:5], kt, want_geometry=True)       # a good call
        assert np.array_equal(out["best_obs"], expect[1][:5]) and out["geometry"].tobytes() == expect[3][:5].tobytes()
        assert pl.a.read(old_slots).tobytes() == want_old.tobytes()
        return str(ei.value)

    def put(i, v, field=None):
        def f(arr):
            if field:
                arr[field][i] = v
            else:
                arr[i] = v
        return f
    refused(INVALID, what=0); refused(INVALID, what=4)
    refused(INVALID, obs_off=put(0, 1)); refused(INVALID, obs_off=put(n, off[n] + 1)); refused(INVALID, obs_off=put(1, off[2] + 1))
    refused(INVALID, mp_slots=put(1, pl.a.capacity)); refused(INVALID, mp_slots=put(1, -1))
    assert "point 3" in refused(INVALID, mp_slots=put(3, slots[0]))         # named twice
    refused(INVALID, mp_slots=put(0, 1))                                    # an old point's slot never written (the gaps)
    refused(INVALID, is_new=put(2, 1))                                      # a new point with N = 0
    refused(INVALID, what=S.DESCRIPTOR); refused(INVALID, what=S.GEOMETRY)  # a new point needs both
    refused(INVALID, obs=put(off[1], 12, "kf")); refused(INVALID, obs=put(off[1], -1, "kf"))
    assert "keyframe 3" in refused(INVALID, kfs=put(3, pl.kf_store.capacity, "slot"))
    refused(INVALID, kfs=put(3, -1, "slot")); refused(INVALID, kfs=put(3, 2, "slot")); refused(INVALID, kfs=put(3, 1, "slot"))      # outside, never written, removed
    refused(INVALID, kfs=put(3, 2, "flags"))
    k0 = int(obs["kf"][off[0]])
    refused(INVALID, obs=put(off[0], len(kfs12[k0]["kps"]), "kp")); refused(INVALID, obs=put(off[0], -1, "kp"))
    refused(INVALID, ref_obs=put(1, 5)); refused(INVALID, ref_obs=put(1, -1))
    refused(INVALID, ref_obs=put(4, gone_at))                               # a bad keyframe without a slot as the ref
    big = np.zeros(513, capi.MP_OBS_DTYPE)
    with pytest.raises(capi.DvmError) as ei:                                # 513 observations
        pl.a.refresh(pl.kf_store, slots[:1], np.array([0, 513], np.int32), big, ref[:1], kt)
    assert ei.value.code == CAPACITY_ERR
    a = capi.MpRefresh(1, len(kt), 3, 3, slots.ctypes.data, None, obs.ctypes.data, ref.ctypes.data, kt.ctypes.data, None, None, np.zeros(1, np.int32).ctypes.data, None, None)
    f = pl.a.L.dvm_map_store_refresh
    assert f(pl.a.h, pl.kf_store.h, C.byref(a)) == INVALID and f(pl.a.h, None, C.byref(a)) == INVALID          # a NULL required array, a NULL store
    if capi.device_count() >= 2:
        far = capi.KeyframeStore(2, 64, device=1)
        with pytest.raises(capi.DvmError) as ei:
            pl.a.refresh(far, slots[:5], off[:6], obs[:off[5]], ref[:5], kt)
        assert ei.value.code == INVALID
        far.close()
    _, out, rec = check(sc, pl=pl)                                          # and the whole call, the new point included
    assert rec["bad"][5] == 0 and out["best_obs"][5] >= 0
    pl.close()


def test_bytes_that_travel(kfs12):
    """up: the arrays given and no more than 256 B each + 1 KiB on top; down: 4 B per point for best_obs, 4 for best_median, 32 for the
    geometry rows when asked for; nothing proportional to 32 B per observation"""
    sc = S.make_scene(29, kfs12, [400, 500, 512, 3, 2, 0], new=[3], distinct=False)
    pl = Placed(sc)
    n, E, K = 6, int(sc["obs_off"][-1]), 12
    payload = 4 * n + 4 * (n + 1) + 8 * E + 4 * n + 20 * K + n + 12 * n
    pl.refresh(want_geometry=True)
    up, down = pl.a.last_refresh_bytes()
    assert payload <= up <= payload + 7 * 256 + 1024, (up, payload)
    assert down == 4 * n + 4 * n + 32 * n
    assert up < 12 * E                                                      # (32 B per observation would be 45 KB)
    sc_old = S.make_scene(29, kfs12, [3, 2, 9], distinct=False)
    pl2 = Placed(sc_old)
    pl2.refresh(want_geometry=False)
    up, down = pl2.a.last_refresh_bytes()
    payload = 4 * 3 + 4 * 4 + 8 * 14 + 4 * 3 + 20 * K
    assert payload <= up <= payload + 5 * 256 + 1024 and down == 4 * 3 + 4 * 3
    pl.close(); pl2.close()
