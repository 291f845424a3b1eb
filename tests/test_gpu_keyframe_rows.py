"""The rows a dvm_keyframe_store keeps beside its keyframes (dvm_keyframe_store_set_rows / _patch_rows / _debug_read_rows): what a set
writes, read back at row lengths 0, 1, 63, 64, 65, 257 and 320 (slot_keypoints 320: a row spans two 256-entry blocks); patches -- single
cells, a cell edited twice in one call, several slots; set and patch queued back to back; put and remove unset a slot's rows; every refusal,
each followed by a good call with the rows as they were; a store without a row call reads as before."""
import ctypes as C

import numpy as np
import pytest

import keyframe_store_scene as kss

pytestmark = pytest.mark.gpu

SLOT_KEYPOINTS, CAPACITY, MAP_CAPACITY = 320, 140, 1000
LENS = (0, 1, 63, 64, 65, 257, 320)
SLOTS = (0, 5, 6, 77, 100, 138, 139)
INVALID, CAPACITY_ERR = -1, -3
WRITTEN = 900                    # map slots [0, WRITTEN) are written


class World:
    def __init__(self, capi):
        self.capi = capi
        self.kfs = capi.KeyframeStore(CAPACITY, SLOT_KEYPOINTS)
        self.points = capi.MapStore(MAP_CAPACITY)
        self.points.update(np.arange(WRITTEN, dtype=np.int32), np.zeros(WRITTEN, capi.LOCAL_POINT_DTYPE))
        self.keyframes = {sl: kss.keyframe(50 + sl, n) for sl, n in zip(SLOTS, LENS)}
        self.kfs.put(list(SLOTS), [self.keyframes[sl] for sl in SLOTS])

    def rows(self, seed):
        rng = np.random.default_rng(seed)
        return [np.where(rng.random(n) < 0.3, -1, rng.integers(0, WRITTEN, n)).astype(np.int32) for n in LENS]

    def close(self):
        self.kfs.close(); self.points.close()


@pytest.fixture(scope="module")
def world(capi):
    w = World(capi)
    yield w
    w.close()


def _read_all(w, which):
    return [w.kfs.read_rows(which, sl) for sl in SLOTS]


def _equal(a, b):
    return len(a) == len(b) and all(x.dtype == np.int32 and np.array_equal(x, y) for x, y in zip(a, b))


def test_a_store_without_a_row_call_reads_as_before(capi):
    st = capi.KeyframeStore(4, SLOT_KEYPOINTS)
    kf = kss.keyframe(3, 257)
    st.put([2], [kf])
    kss.assert_slot_is(st.read(2), kf)
    for which in (capi.KFS_ROW_MATCHES, capi.KFS_ROW_OBSERVED):
        assert len(st.read_rows(which, 2)) == 0
    st.close()


def test_set_then_read_back(capi, world):
    for which, seed in ((capi.KFS_ROW_MATCHES, 1), (capi.KFS_ROW_OBSERVED, 2)):
        rows = world.rows(seed)
        world.kfs.set_rows(which, world.points, list(SLOTS), rows)
        assert _equal(_read_all(world, which), rows)
        assert world.kfs.last_put_bytes() >= sum(4 * n for n in LENS)
    # the two kinds are independent, and a second set replaces the first
    assert _equal(_read_all(world, capi.KFS_ROW_MATCHES), world.rows(1))
    rows = world.rows(3)
    world.kfs.set_rows(capi.KFS_ROW_MATCHES, world.points, [SLOTS[5], SLOTS[2]], [rows[5], rows[2]])
    want = world.rows(1); want[5], want[2] = rows[5], rows[2]
    assert _equal(_read_all(world, capi.KFS_ROW_MATCHES), want)
    assert _equal(_read_all(world, capi.KFS_ROW_OBSERVED), world.rows(2))


def test_patch(capi, world):
    M = capi.KFS_ROW_MATCHES
    rows = world.rows(4)
    world.kfs.set_rows(M, world.points, list(SLOTS), rows)
    world.kfs.patch_rows(M, world.points, [(SLOTS[6], 319, 7)])                       # a single cell, the last of the longest row
    rows[6][319] = 7
    assert _equal(_read_all(world, M), rows)
    # a cell edited twice (the last wins), edits in several slots, -1 written
    edits = [(SLOTS[5], 256, 11), (SLOTS[1], 0, 12), (SLOTS[5], 256, 13), (SLOTS[3], 63, -1), (SLOTS[5], 0, 14), (SLOTS[1], 0, -1), (SLOTS[1], 0, 15)]
    world.kfs.patch_rows(M, world.points, edits)
    rows[5][256], rows[1][0], rows[3][63], rows[5][0] = 13, 15, -1, 14
    assert _equal(_read_all(world, M), rows)
    assert world.kfs.last_put_bytes() == 12 * 4                                      # four cells travel


def test_set_and_patch_back_to_back(capi, world):
    O = capi.KFS_ROW_OBSERVED
    a, b = world.rows(5), world.rows(6)
    world.kfs.set_rows(O, world.points, list(SLOTS), a)
    world.kfs.patch_rows(O, world.points, [(SLOTS[4], k, 100 + k) for k in range(65)])
    world.kfs.set_rows(O, world.points, [SLOTS[2]], [b[2]])
    world.kfs.patch_rows(O, world.points, [(SLOTS[2], 62, 5), (SLOTS[4], 64, 6)])
    a[4] = (100 + np.arange(65)).astype(np.int32); a[4][64] = 6
    a[2] = b[2].copy(); a[2][62] = 5
    assert _equal(_read_all(world, O), a)


def test_a_patch_opens_a_row_that_is_not_set(capi):
    st = capi.KeyframeStore(3, SLOT_KEYPOINTS)
    pts = capi.MapStore(8)
    pts.update([0, 1, 2], np.zeros(3, capi.LOCAL_POINT_DTYPE))
    st.put([1], [kss.keyframe(4, 65)])
    st.patch_rows(capi.KFS_ROW_OBSERVED, pts, [(1, 64, 2), (1, 3, 0)])
    want = np.full(65, -1, np.int32); want[64], want[3] = 2, 0
    assert np.array_equal(st.read_rows(capi.KFS_ROW_OBSERVED, 1), want)
    assert len(st.read_rows(capi.KFS_ROW_MATCHES, 1)) == 0
    st.close(); pts.close()


def test_put_and_remove_unset_the_rows(capi, world):
    M, O = capi.KFS_ROW_MATCHES, capi.KFS_ROW_OBSERVED
    rows = world.rows(7)
    # every point voted for once per entry: the votes of a slot are its row's entries that name a point
    for which in (M, O):
        world.kfs.set_rows(which, world.points, list(SLOTS), rows)
    ulm = capi.UpdateLocalMap()
    ulm.reserve(1, 1024, 8, MAP_CAPACITY, CAPACITY, SLOT_KEYPOINTS)
    frame = dict(kfs=world.kfs, points=world.points, mp_slot=np.arange(WRITTEN, dtype=np.int32))
    votes = ulm.keyframes([frame])[0]["votes"]
    for sl, r in zip(SLOTS, rows):
        assert votes[sl] == (r >= 0).sum()
    assert ulm.points([dict(frame, kf_slot=[SLOTS[5], SLOTS[4]])])[0]["n_local"] > 0
    # a put to SLOTS[5], a remove of SLOTS[4]: no rows, no votes, and _points refuses the slots
    world.kfs.put([SLOTS[5]], [world.keyframes[SLOTS[5]]])
    world.kfs.remove([SLOTS[4]])
    assert len(world.kfs.read_rows(M, SLOTS[5])) == 0 and len(world.kfs.read_rows(O, SLOTS[5])) == 0
    votes = ulm.keyframes([frame])[0]["votes"]
    assert votes[SLOTS[5]] == 0 and votes[SLOTS[4]] == 0 and votes[SLOTS[6]] == (rows[6] >= 0).sum()
    for sl, what in ((SLOTS[5], "without a MATCHES row"), (SLOTS[4], "never put or removed")):
        with pytest.raises(capi.DvmError) as e:
            ulm.points([dict(frame, kf_slot=[SLOTS[6], sl])])
        assert e.value.code == INVALID and what in str(e.value) and "entry 1" in str(e.value)
    # the removed slot put again holds nothing until it is told
    world.kfs.put([SLOTS[4]], [world.keyframes[SLOTS[4]]])
    assert ulm.keyframes([frame])[0]["votes"][SLOTS[4]] == 0
    world.kfs.set_rows(O, world.points, [SLOTS[4]], [rows[4]])
    assert ulm.keyframes([frame])[0]["votes"][SLOTS[4]] == (rows[4] >= 0).sum()
    ulm.close()


def test_put_device_unsets_the_rows(capi):
    """dvm_keyframe_store_put_device (the body of put_tracked too) on a slot whose rows are set: no rows, no votes, a neighbour's rows kept."""
    import test_gpu_keyframe_put_device as pdv
    M, O = capi.KFS_ROW_MATCHES, capi.KFS_ROW_OBSERVED
    st = capi.KeyframeStore(4, SLOT_KEYPOINTS)
    pts = capi.MapStore(16)
    pts.update(np.arange(8, dtype=np.int32), np.zeros(8, capi.LOCAL_POINT_DTYPE))
    voc = capi.Vocabulary(pdv.vocabulary("full"))
    st.put([1, 2], [kss.keyframe(60, 257), kss.keyframe(61, 65)])
    rows = [np.arange(257, dtype=np.int32) % 8, np.arange(65, dtype=np.int32) % 8]
    for which in (M, O):
        st.set_rows(which, pts, [1, 2], rows)
    ulm = capi.UpdateLocalMap()
    ulm.reserve(1, 16, 4, 16, 4, SLOT_KEYPOINTS)
    frame = dict(kfs=st, points=pts, mp_slot=np.arange(8, dtype=np.int32))
    assert list(ulm.keyframes([frame])[0]["votes"]) == [0, 257, 65, 0]
    kps, desc = pdv.arrays(257, 3)
    st.put_device(voc, [1], [pdv.dev_kf(kps, desc)], levelsup=2)
    assert list(ulm.keyframes([frame])[0]["votes"]) == [0, 0, 65, 0]                  # nothing synchronised by the test in between
    assert len(st.read_rows(M, 1)) == 0 and len(st.read_rows(O, 1)) == 0 and np.array_equal(st.read_rows(M, 2), rows[1])
    with pytest.raises(capi.DvmError) as e:
        ulm.points([dict(frame, kf_slot=[2, 1])])
    assert e.value.code == INVALID and "without a MATCHES row" in str(e.value)
    st.set_rows(O, pts, [1], [rows[0]])                                              # told again, it votes again
    assert list(ulm.keyframes([frame])[0]["votes"]) == [0, 257, 65, 0]
    ulm.close(); voc.close(); st.close(); pts.close()


def test_null_arguments_and_removed_slots(capi, world):
    M = capi.KFS_ROW_MATCHES
    rows = world.rows(10)
    world.kfs.set_rows(M, world.points, list(SLOTS), rows)
    L = capi.lib()
    slots = np.array([SLOTS[2]], np.int32)
    edit = np.array([(SLOTS[2], 0, 1)], capi.KFS_ROW_EDIT_DTYPE)
    n_out = np.zeros(1, np.int32)
    for rc in (L.dvm_keyframe_store_set_rows(world.kfs.h, M, world.points.h, 1, None, None),
               L.dvm_keyframe_store_set_rows(world.kfs.h, M, world.points.h, 1, slots.ctypes.data, None),
               L.dvm_keyframe_store_set_rows(None, M, world.points.h, 1, slots.ctypes.data, None),
               L.dvm_keyframe_store_patch_rows(world.kfs.h, M, world.points.h, 1, None),
               L.dvm_keyframe_store_patch_rows(None, M, world.points.h, 1, edit.ctypes.data),
               L.dvm_keyframe_store_set_rows(world.kfs.h, M, world.points.h, -1, slots.ctypes.data, None),
               L.dvm_keyframe_store_debug_read_rows(world.kfs.h, M, SLOTS[2], None, 8, n_out.ctypes.data)):
        assert rc == INVALID
    assert L.dvm_keyframe_store_set_rows(world.kfs.h, M, world.points.h, 0, None, None) == 0      # a zero count needs no array
    # a removed slot is refused by both calls, second in a batch: the first is not written either
    gone = 50
    world.kfs.put([gone], [kss.keyframe(9, 64)])
    world.kfs.set_rows(M, world.points, [gone], [np.zeros(64, np.int32)])
    world.kfs.remove([gone])
    for call in (lambda: world.kfs.set_rows(M, world.points, [SLOTS[2], gone], [world.rows(11)[2], np.zeros(64, np.int32)]),
                 lambda: world.kfs.patch_rows(M, world.points, [(SLOTS[2], 0, 5), (gone, 0, 1)])):
        with pytest.raises(capi.DvmError) as e:
            call()
        assert e.value.code == INVALID and "slot %d" % gone in str(e.value) and "removed" in str(e.value)
        assert _equal(_read_all(world, M), rows)
    with pytest.raises(capi.DvmError):
        world.kfs.read_rows(M, gone)
    # the update-local-map calls with a NULL array and a non-zero count
    ulm = capi.UpdateLocalMap()
    ulm.reserve(1, 16, 4, MAP_CAPACITY, CAPACITY, SLOT_KEYPOINTS)
    assert L.dvm_update_local_map_keyframes(ulm.h, 1, None, None) == INVALID
    assert L.dvm_update_local_map_points(ulm.h, 1, None, None) == INVALID
    ki = capi._UlmKeyframesIn(world.kfs.h, world.points.h, 3, None); ko = capi._UlmKeyframesOut(None, None)
    assert L.dvm_update_local_map_keyframes(ulm.h, 1, C.addressof(ki), C.addressof(ko)) == INVALID
    votes = np.zeros(CAPACITY, np.int32); bad = np.zeros(4, np.uint8)
    ko = capi._UlmKeyframesOut(votes.ctypes.data, bad.ctypes.data)
    assert L.dvm_update_local_map_keyframes(ulm.h, 1, C.addressof(ki), C.addressof(ko)) == INVALID      # mp_slot NULL, n = 3
    assert "NULL" in L.dvm_last_error().decode()
    pi = capi._UlmPointsIn(world.kfs.h, world.points.h, 2, None, 0, None); po = capi._UlmPointsOut(None, 0, -7, None, -7)
    assert L.dvm_update_local_map_points(ulm.h, 1, C.addressof(pi), C.addressof(po)) == INVALID         # kf_slot NULL, n_kfs = 2
    assert L.dvm_update_local_map_keyframes(ulm.h, 0, None, None) == 0
    assert ulm.keyframes([dict(kfs=world.kfs, points=world.points, mp_slot=np.zeros(0, np.int32))])[0]["votes"].shape == (CAPACITY,)
    ulm.close()


def test_refusals_leave_the_rows_as_they_were(capi, world):
    M = capi.KFS_ROW_MATCHES
    rows = world.rows(8)
    world.kfs.set_rows(M, world.points, list(SLOTS), rows)
    good = world.rows(9)
    n5 = LENS[5]

    def damaged(at, value):
        r = good[5].copy(); r[at] = value
        return r
    far = None
    if capi.device_count() > 1:
        far = capi.MapStore(4, device=1)
    empty = 1                                                                        # a slot never put
    cases = [
        ("slot outside", lambda: world.kfs.set_rows(M, world.points, [SLOTS[2], CAPACITY], [good[2], good[2]]), "row 1 (slot %d)" % CAPACITY),
        ("slot negative", lambda: world.kfs.set_rows(M, world.points, [SLOTS[2], -1], [good[2], good[2]]), "row 1 (slot -1)"),
        ("slot never put", lambda: world.kfs.set_rows(M, world.points, [SLOTS[2], empty], [good[2], good[2]]), "row 1 (slot 1)"),
        ("NULL row", lambda: world.kfs.set_rows(M, world.points, [SLOTS[2], SLOTS[5]], [good[2], None]), "NULL row"),
        ("value below -1", lambda: world.kfs.set_rows(M, world.points, [SLOTS[2], SLOTS[5]], [good[2], damaged(n5 - 1, -2)]), "entry %d = -2" % (n5 - 1)),
        ("value outside", lambda: world.kfs.set_rows(M, world.points, [SLOTS[2], SLOTS[5]], [good[2], damaged(0, MAP_CAPACITY)]), "entry 0 = %d" % MAP_CAPACITY),
        ("value never written", lambda: world.kfs.set_rows(M, world.points, [SLOTS[2], SLOTS[5]], [good[2], damaged(7, WRITTEN)]), "entry 7 = %d" % WRITTEN),
        ("slot twice", lambda: world.kfs.set_rows(M, world.points, [SLOTS[2], SLOTS[3], SLOTS[2]], [good[2], good[3], good[2]]), "named twice"),
        ("which", lambda: world.kfs.set_rows(2, world.points, [SLOTS[2]], [good[2]]), "which = 2"),
        ("no map store", lambda: world.kfs.set_rows(M, None, [SLOTS[2]], [good[2]]), "missing map store"),
        ("patch kp outside", lambda: world.kfs.patch_rows(M, world.points, [(SLOTS[2], 0, 1), (SLOTS[2], LENS[2], 1)]), "edit 1 (slot %d, kp %d)" % (SLOTS[2], LENS[2])),
        ("patch kp negative", lambda: world.kfs.patch_rows(M, world.points, [(SLOTS[2], 0, 1), (SLOTS[2], -1, 1)]), "kp outside"),
        ("patch kp of an empty row", lambda: world.kfs.patch_rows(M, world.points, [(SLOTS[0], 0, 1)]), "kp outside [0, 0)"),
        ("patch slot never put", lambda: world.kfs.patch_rows(M, world.points, [(SLOTS[2], 0, 1), (empty, 0, 1)]), "edit 1 (slot 1"),
        ("patch value never written", lambda: world.kfs.patch_rows(M, world.points, [(SLOTS[2], 0, 1), (SLOTS[2], 1, WRITTEN)]), "value %d" % WRITTEN),
        ("patch value below -1", lambda: world.kfs.patch_rows(M, world.points, [(SLOTS[2], 0, 1), (SLOTS[2], 1, -5)]), "value -5"),
    ]
    if far is not None:
        cases.append(("points on another device", lambda: world.kfs.set_rows(M, far, [SLOTS[2]], [good[2]]), "another device"))
    other = capi.MapStore(WRITTEN)
    other.update(np.arange(4, dtype=np.int32), np.zeros(4, capi.LOCAL_POINT_DTYPE))
    cases.append(("patch of a row that names another store", lambda: world.kfs.patch_rows(M, other, [(SLOTS[2], 0, 1)]), "another map store"))
    for name, call, text in cases:
        with pytest.raises(capi.DvmError) as e:
            call()
        assert e.value.code == INVALID and text in str(e.value), (name, str(e.value))
        assert _equal(_read_all(world, M), rows), name
    # a good call after them
    world.kfs.patch_rows(M, world.points, [(SLOTS[2], 0, 1)])
    rows[2][0] = 1
    assert _equal(_read_all(world, M), rows)
    with pytest.raises(capi.DvmError) as e:
        world.kfs.read_rows(M, empty)
    assert e.value.code == INVALID
    other.close()
    if far is not None:
        far.close()
