"""dvm_keyframe_store: what put writes to a slot, read back through debug_read and compared byte for byte with the keyframe and with
the grid restated in numpy (tests/keyframe_store_scene.grid_of).  Sizes: the tails of k_kfs_put's 1 024-thread workgroup (0, 1, 1 023,
1 024, 1 025) and n == slot_keypoints; batches, overwriting, remove, a put in several staging rounds, and every error of put, each
leaving the store as it was."""
import numpy as np
import pytest

import keyframe_store_scene as kss

pytestmark = pytest.mark.gpu

SLOT_KEYPOINTS = 1100
CAPACITY = 6
INVALID, CAPACITY_ERR = -1, -3


@pytest.fixture(scope="module")
def store(capi):
    st = capi.KeyframeStore(CAPACITY, SLOT_KEYPOINTS)
    yield st
    st.close()


def test_create_arguments(capi, store):
    assert store.capacity == CAPACITY and store.slot_keypoints == SLOT_KEYPOINTS
    for cap, k in ((0, 64), (4, 0), (4, 8193)):
        with pytest.raises(capi.DvmError) as e:
            capi.KeyframeStore(cap, k)
        assert e.value.code == INVALID


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, SLOT_KEYPOINTS])
def test_round_trip(store, n):
    kf = kss.keyframe(1, n)
    store.put([3], [kf])
    r = store.read(3)
    kss.assert_slot_is(r, kf)
    if n >= 1023:
        assert 0.8 * n < r["n_sorted"] < n                       # some keypoints lie outside the grid


def test_batch_to_non_adjacent_slots_in_one_call(store):
    kfs = [kss.keyframe(2, 700), kss.keyframe(3, 64, fv=False), kss.keyframe(4, 1025)]
    store.put([5, 0, 2], kfs)
    for sl, kf in zip((5, 0, 2), kfs):
        kss.assert_slot_is(store.read(sl), kf)


def test_overwrite_with_a_smaller_keyframe(store):
    big, small = kss.keyframe(5, SLOT_KEYPOINTS), kss.keyframe(6, 200)
    store.put([1], [big])
    g0 = store.read(1)["generation"]
    kss.assert_slot_is(store.read(1), big)
    store.put([1], [small])
    r = store.read(1)
    kss.assert_slot_is(r, small)                                 # counters, cell_start and every array are the small keyframe's
    assert r["generation"] == g0 + 1 and r["cell_start"][kss.GRID_COLS * kss.GRID_ROWS] == r["n_sorted"] <= 200
    assert len(r["kps"]) == 200 and len(r["sidx"]) == r["n_sorted"] and r["sidx"].max() < 200
    fresh = kss.keyframe(6, 200)
    store.put([4], [fresh])                                      # a slot that never held the large one reads the same
    a, b = store.read(1), store.read(4)
    for k in ("kps", "desc", "fv_nodes", "fv_off", "fv_feat", "skp", "sidx", "sdesc"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(a["cell_start"][:3073], b["cell_start"][:3073])


def test_remove(capi, store):
    kf = kss.keyframe(7, 300)
    store.put([0, 2], [kf, kf])
    g = store.read(2)["generation"]
    store.remove([2])
    with pytest.raises(capi.DvmError) as e:
        store.read(2)
    assert e.value.code == INVALID
    kss.assert_slot_is(store.read(0), kf)                        # the other slot stays
    for bad in ([2], [CAPACITY], [-1], [0, 2]):                  # not written, outside; a call with one bad slot removes nothing
        with pytest.raises(capi.DvmError) as e:
            store.remove(bad)
        assert e.value.code == INVALID
    kss.assert_slot_is(store.read(0), kf)
    store.put([2], [kf])
    assert store.read(2)["generation"] == g + 2                  # remove and put each bump it


def test_put_in_several_staging_rounds(capi):
    """40 keyframes of the slot size in one call: more than one staging block holds (32 of the largest size)."""
    st = capi.KeyframeStore(40, 64)
    kfs = [kss.keyframe(100 + i, 64 if i % 3 else 40) for i in range(40)]
    st.put(np.arange(40)[::-1], kfs)
    for i in (0, 1, 30, 31, 32, 33, 39):
        kss.assert_slot_is(st.read(39 - i), kfs[i])
    st.close()


def _bad_keyframes():
    """name -> (keyframe dict, a function that damages the dvm_kfs_keyframe struct or None, expected code)"""
    base = kss.keyframe(8, 500)
    fv = base["fv"]

    def with_fv(**kw):
        return dict(base, fv=dict(fv, **kw))
    oct_bad = base["kps"].copy(); oct_bad["octave"][123] = kss.L
    off0 = fv["fv_off"].copy(); off0[0] = 1
    off_dec = fv["fv_off"].copy(); off_dec[3] = off_dec[4] + 1
    feat_hi = fv["fv_feat"].copy(); feat_hi[17] = 500
    feat_neg = fv["fv_feat"].copy(); feat_neg[0] = -1
    nodes = fv["fv_nodes"].copy(); nodes[[0, len(nodes) - 1]] = nodes[[len(nodes) - 1, 0]]          # -1 (last as unsigned) moved to the front
    long_tab = (np.float32(1.01) ** np.arange(65)).astype(np.float32)
    empty = np.zeros(0, np.float32)

    def null(field):
        def f(s):
            setattr(s, field, None)
        return f
    return {
        "n_beyond_the_slot": (kss.keyframe(9, SLOT_KEYPOINTS + 1), None, CAPACITY_ERR),
        "octave_outside_the_tables": (dict(base, kps=oct_bad), None, INVALID),
        "no_levels": (dict(base, scale_factors=empty, level_sigma2=empty, inv_level_sigma2=empty), None, INVALID),
        "65_levels": (dict(base, scale_factors=long_tab, level_sigma2=long_tab, inv_level_sigma2=long_tab), None, INVALID),
        "empty_bounds_x": (dict(base, bounds=np.array([640.0, 640.0, 0.0, 480.0], np.float32)), None, INVALID),
        "empty_bounds_y": (dict(base, bounds=np.array([0.0, 640.0, 480.0, 0.0], np.float32)), None, INVALID),
        "fv_off_not_from_0": (with_fv(fv_off=off0), None, INVALID),
        "fv_off_not_monotone": (with_fv(fv_off=off_dec), None, INVALID),
        "feature_beyond_n": (with_fv(fv_feat=feat_hi), None, INVALID),
        "feature_negative": (with_fv(fv_feat=feat_neg), None, INVALID),
        "nodes_not_ascending_as_unsigned": (with_fv(fv_nodes=nodes), None, INVALID),
        "no_keypoints_array": (base, null("kps"), INVALID),
        "no_descriptors": (base, null("desc"), INVALID),
        "no_scale_factors": (base, null("scale_factors"), INVALID),
        "no_level_sigma2": (base, null("level_sigma2"), INVALID),
        "no_inv_level_sigma2": (base, null("inv_level_sigma2"), INVALID),
        "no_fv_feat": (base, null("fv_feat"), INVALID),
        "no_fv_off": (base, null("fv_off"), INVALID),
    }


BAD = _bad_keyframes()


def _snapshot(store, slots):
    return {sl: store.read(sl) for sl in slots}


def _assert_unchanged(store, before):
    for sl, a in before.items():
        b = store.read(sl)
        assert a["generation"] == b["generation"] and a["n"] == b["n"] and a["n_sorted"] == b["n_sorted"]
        for k in ("kps", "desc", "fv_nodes", "fv_off", "fv_feat", "scale_factors", "level_sigma2", "inv_level_sigma2", "skp", "sidx", "sdesc", "cell_start"):
            assert a[k].tobytes() == b[k].tobytes(), (sl, k)


@pytest.mark.parametrize("name", list(BAD))
def test_a_refused_put_leaves_the_store_unchanged(capi, store, name):
    kf, damage, code = BAD[name]
    good = kss.keyframe(10, 900)
    store.put([1, 4], [good, kss.keyframe(11, 333)])
    before = _snapshot(store, (1, 4))
    # the bad keyframe second in a batch of two: the good one before it is not written either
    arr, keep = store.records([kss.keyframe(12, 50), kf])
    if damage:
        damage(arr[1])
    with pytest.raises(capi.DvmError) as e:
        store.put_raw(np.array([4, 1], np.int32), arr)
    assert e.value.code == code and "keyframe 1 (slot 1)" in str(e.value)
    _assert_unchanged(store, before)
    kss.assert_slot_is(store.read(1), good)


@pytest.mark.parametrize("slots", [[1, CAPACITY], [1, -1], [4, 1, 4]], ids=("beyond_capacity", "negative", "named_twice"))
def test_a_refused_slot_list_leaves_the_store_unchanged(capi, store, slots):
    store.put([1, 4], [kss.keyframe(10, 900), kss.keyframe(11, 333)])
    before = _snapshot(store, (1, 4))
    with pytest.raises(capi.DvmError) as e:
        store.put(slots, [kss.keyframe(13 + i, 80) for i in range(len(slots))])
    assert e.value.code == INVALID and f"keyframe {len(slots) - 1} (slot {slots[-1]})" in str(e.value)
    _assert_unchanged(store, before)
    with pytest.raises(capi.DvmError) as e:
        store.read(CAPACITY)
    assert e.value.code == INVALID
