"""dvm_update_local_map_keyframes: the votes of UpdateLocalKeyFrames and frame_bad against the reference's loop restated in
tests/local_map_scene.py, integer equality.  slot_keypoints 320 (a row spans two 256-entry blocks), keyframe capacity 140, map capacity
1 000.  Frame sizes 0, 1, 63, 64, 65, 257, 1 025; stores with 1, 4, 5, 65, 129 live keyframes with gaps and a removed slot between them and
rows of lengths 0 .. 320, so the tails of the 16-byte loads and of the wave both occur; multiplicity 2 and 3, all -1, all bad; batches of 1
and 3 frames on three different store pairs; ordering behind an update and a patch with nothing synchronised between; idle tables; every
refusal; the byte counter against the header's formula."""
import numpy as np
import pytest

import local_map_scene as lms

pytestmark = pytest.mark.gpu

SLOT_KEYPOINTS, KF_CAPACITY, MAP_CAPACITY = 320, 140, 1000
ROW_LENS = (0, 1, 63, 64, 65, 257, 320, 3, 4, 5, 127, 128, 129, 255, 256, 319)
FRAME_NS = (0, 1, 63, 64, 65, 257, 1025)
INVALID, CAPACITY_ERR = -1, -3


def _graph(seed, n_live, frame_n, **kw):
    rng = np.random.default_rng(seed)
    slots = np.sort(rng.permutation(KF_CAPACITY - 1)[:n_live])                      # gaps between them; slot 139 stays free
    lens = [ROW_LENS[(i + seed) % len(ROW_LENS)] for i in range(n_live)]
    a = dict(kf_slots=slots, row_lens=lens, n_points=600, frame_n=frame_n, map_capacity=MAP_CAPACITY, kf_capacity=KF_CAPACITY,
             slot_keypoints=SLOT_KEYPOINTS, fill=0.7)
    a.update(kw)
    return lms.make_graph(seed, **a)


@pytest.fixture(scope="module")
def ulm(capi):
    u = capi.UpdateLocalMap()
    u.reserve(3, 1025, 129, MAP_CAPACITY, KF_CAPACITY, SLOT_KEYPOINTS)
    yield u
    u.close()


def _check(res, g):
    votes, frame_bad = lms.reference_keyframes(g)
    assert res["votes"].dtype == np.int32 and np.array_equal(res["votes"], votes)
    assert np.array_equal(res["frame_bad"], frame_bad)
    assert (res["votes_guarded"][len(votes):] == -7).all() and (res["frame_bad_guarded"][len(frame_bad):] == 7).all()


@pytest.fixture(scope="module")
def placed(capi):
    """Stores of 1, 4, 5, 65 and 129 live keyframes, each with a removed slot whose rows had been set."""
    out = {}
    for n_live in (1, 4, 5, 65, 129):
        g = _graph(n_live, n_live, 257)
        p = lms.Placed(capi, g)
        import keyframe_store_scene as kss
        extra = KF_CAPACITY - 1                                                      # a keyframe with rows, then removed: its device length is 0 again
        p.kfs.put([extra], [kss.keyframe(7, 320)])
        p.kfs.set_rows(capi.KFS_ROW_OBSERVED, p.points, [extra], [np.full(320, g.points[0].slot, np.int32)])
        p.kfs.remove([extra])
        out[n_live] = p
    yield out
    for p in out.values():
        p.close()


@pytest.mark.parametrize("n_live", [1, 4, 5, 65, 129])
def test_votes_on_stores_of_several_sizes(ulm, placed, n_live):
    p = placed[n_live]
    _check(ulm.keyframes([p.frame_keyframes()])[0], p.g)
    assert lms.reference_keyframes(p.g)[0].any()


@pytest.mark.parametrize("n", FRAME_NS)
def test_frame_sizes(ulm, placed, n):
    p = placed[65]
    rng = np.random.default_rng(n)
    pts = p.g.points
    p.g.frame = [None if rng.random() < 0.1 else pts[int(rng.integers(len(pts)))] for _ in range(n)]
    _check(ulm.keyframes([p.frame_keyframes()])[0], p.g)


def test_multiplicity_all_none_all_bad(capi, ulm, placed):
    p = placed[5]
    g = p.g
    live = [q for q in g.points if not q.bad and q.observations]
    bad = [q for q in g.points if q.bad]
    assert live and bad
    g.frame = [live[0], live[1], live[0], None, live[0], live[1]]                    # multiplicity 3 and 2
    res = ulm.keyframes([p.frame_keyframes()])[0]
    _check(res, g)
    for kf in g.kfs:
        assert res["votes"][kf.slot] == 3 * (kf in live[0].observations) + 2 * (kf in live[1].observations)
    g.frame = [None] * 65
    res = ulm.keyframes([p.frame_keyframes()])[0]
    _check(res, g)
    assert not res["votes"].any() and not res["frame_bad"].any()
    g.frame = [bad[i % len(bad)] for i in range(65)]
    res = ulm.keyframes([p.frame_keyframes()])[0]
    _check(res, g)
    assert not res["votes"].any() and res["frame_bad"].all()


def test_batch_of_three_store_pairs(ulm, placed):
    ps = [placed[129], placed[4], placed[65]]
    for p, n in zip(ps, (257, 0, 1025)):
        rng = np.random.default_rng(n + 1)
        p.g.frame = [p.g.points[int(rng.integers(len(p.g.points)))] for _ in range(n)]
    single = [ulm.keyframes([p.frame_keyframes()])[0] for p in ps]
    batch = ulm.keyframes([p.frame_keyframes() for p in ps])
    up, down = ulm.last_bytes()
    assert up == 64 * 3 + sum(4 * ((n + 15) // 16 * 16) for n in (257, 0, 1025))    # the header's formula
    assert down == sum(4 * KF_CAPACITY + n for n in (257, 0, 1025))
    for p, s, b in zip(ps, single, batch):
        _check(b, p.g)
        assert np.array_equal(s["votes"], b["votes"]) and np.array_equal(s["frame_bad"], b["frame_bad"])
    # the same store pair in two frames of one call
    two = ulm.keyframes([ps[0].frame_keyframes(), ps[0].frame_keyframes()])
    assert np.array_equal(two[0]["votes"], two[1]["votes"]) and np.array_equal(two[0]["votes"], single[0]["votes"])


def test_ordering_behind_an_update_and_a_patch(capi, ulm, placed):
    """dvm_map_store_update that sets bad, then the votes; patch_rows, then the votes: nothing synchronised between."""
    p = placed[65]
    g = p.g
    live = [q for q in g.points if not q.bad and q.observations]
    g.frame = live[:40] + live[:10]
    before = ulm.keyframes([p.frame_keyframes()])[0]
    _check(before, g)
    flip = live[:10]
    for q in flip:
        q.bad = True
    rec = np.zeros(len(flip), capi.LOCAL_POINT_DTYPE); rec["bad"] = 1
    p.points.update([q.slot for q in flip], rec)
    after = ulm.keyframes([p.frame_keyframes()])[0]
    _check(after, g)
    assert after["frame_bad"].sum() == 20 and not np.array_equal(after["votes"], before["votes"])
    # an observation erased and one added (EraseObservation / AddObservation as row edits)
    q = live[20]
    kf_old, kp_old = next(iter(q.observations.items()))
    kf_new = next(kf for kf in g.kfs if kf not in q.observations and len(kf.matches) > 0)
    del q.observations[kf_old]
    q.observations[kf_new] = 0
    for other in g.points:                                                           # the cell's former owner loses its observation
        if other is not q and other.observations.get(kf_new) == 0:
            del other.observations[kf_new]
    p.kfs.patch_rows(capi.KFS_ROW_OBSERVED, p.points, [(kf_old.slot, kp_old, -1), (kf_new.slot, 0, q.slot)])
    patched = ulm.keyframes([p.frame_keyframes()])[0]
    _check(patched, g)
    assert patched["votes"][kf_old.slot] == after["votes"][kf_old.slot] - 1
    assert np.array_equal(p.kfs.read_rows(capi.KFS_ROW_OBSERVED, kf_new.slot), lms.row_observed(kf_new, g.points))


def test_identical_calls_and_idle_tables_behind_a_refusal(capi, ulm, placed):
    p = placed[129]
    a = ulm.keyframes([p.frame_keyframes()])[0]
    with pytest.raises(capi.DvmError):
        ulm.keyframes([p.frame_keyframes(), p.frame_keyframes(np.array([0, MAP_CAPACITY], np.int32))])
    b = ulm.keyframes([p.frame_keyframes()])[0]
    c = ulm.keyframes([p.frame_keyframes()])[0]
    assert np.array_equal(a["votes"], b["votes"]) and np.array_equal(b["votes"], c["votes"]) and np.array_equal(a["frame_bad"], c["frame_bad"])
    _check(c, p.g)


def test_refusals(capi, ulm, placed):
    p, q = placed[5], placed[4]
    ok = p.frame_keyframes()
    unwritten = next(s for s in range(MAP_CAPACITY) if s not in {x.slot for x in p.g.points})
    cases = [
        ("slot below -1", [ok, p.frame_keyframes(np.array([0, -2], np.int32))], INVALID, "frame 1, entry 1 (slot -2)"),
        ("slot outside", [p.frame_keyframes(np.array([MAP_CAPACITY], np.int32))], INVALID, "frame 0, entry 0"),
        ("slot never written", [p.frame_keyframes(np.array([-1, unwritten], np.int32))], INVALID, "frame 0, entry 1 (slot %d)" % unwritten),
        ("OBSERVED rows of another map", [dict(kfs=p.kfs, points=q.points, mp_slot=np.zeros(0, np.int32))], INVALID, "another map store"),
        ("too many frames", [ok] * 4, CAPACITY_ERR, "max_frames"),
        ("too many keypoints", [p.frame_keyframes(np.full(1026, -1, np.int32))], CAPACITY_ERR, "max_frame_keypoints"),
    ]
    for name, frames, code, text in cases:
        with pytest.raises(capi.DvmError) as e:
            ulm.keyframes(frames)
        assert e.value.code == code and text in str(e.value), (name, str(e.value))
        _check(ulm.keyframes([ok])[0], p.g)
    small = capi.UpdateLocalMap()
    with pytest.raises(capi.DvmError) as e:                                          # nothing reserved
        small.keyframes([ok])
    assert e.value.code == CAPACITY_ERR
    for sizes, text in (((1, 1025, 8, MAP_CAPACITY - 1, KF_CAPACITY, SLOT_KEYPOINTS), "map_capacity"),
                        ((1, 1025, 8, MAP_CAPACITY, KF_CAPACITY - 1, SLOT_KEYPOINTS), "kf_capacity"),
                        ((1, 1025, 8, MAP_CAPACITY, KF_CAPACITY, SLOT_KEYPOINTS - 1), "slot_keypoints")):
        u = capi.UpdateLocalMap()
        u.reserve(*sizes)
        with pytest.raises(capi.DvmError) as e:
            u.keyframes([ok])
        assert e.value.code == CAPACITY_ERR and text in str(e.value)
        u.close()
    small.reserve(1, 16, 1, MAP_CAPACITY, KF_CAPACITY, SLOT_KEYPOINTS)
    small.reserve(1, 8, 0, 10, 10, 64)                                               # grow-only: a smaller reservation changes nothing
    p.g.frame = p.g.frame[:16]
    _check(small.keyframes([p.frame_keyframes()])[0], p.g)
    assert small.keyframes([]) == []
    small.close()
    if capi.device_count() > 1:
        far = capi.MapStore(4, device=1)
        with pytest.raises(capi.DvmError) as e:
            ulm.keyframes([dict(kfs=p.kfs, points=far, mp_slot=np.zeros(0, np.int32))])
        assert e.value.code == INVALID and "another device" in str(e.value)
        far.close()
