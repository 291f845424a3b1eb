"""dvm_search_by_bow_targets_resident: the place-recognition BoW searches on keyframes that live in a dvm_keyframe_store, their map
points in dvm_map_stores.  The search and settle kernels are the uploaded call's, so every comparison is array_equal against
BowTargets.search on the same keyframes, where the uploaded call carries mp = mp_slot and bad = the record's bad.  The scenes are
tests/bow_targets_scene.py's; on top of them the prologue kernel's edges (keyframe sizes around its workgroup of 256 threads x 4
keypoints, fv_n = 0, no point, every point bad, features no node lists), slots in any order and named more than once, a second map
store, the ordering against update and put with no synchronisation in between, every refusal, and the upload counter against the
header's formula."""
import numpy as np
import pytest

import bow_targets_scene as bts

pytestmark = pytest.mark.gpu

SLOT_KEYPOINTS = 1100
CAPACITY = 16
POINTS = 1 << 15
INVALID, CAPACITY_ERR = -1, -3
WG_THREADS, WG_SPAN = 256, 1024          # k_bt_prologue: threads of a workgroup, keypoints it covers (bow_targets_kernels.h)
SF = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
LEVELS = dict(K=np.array([500.0, 500.0, 320.0, 240.0], np.float32), scale_factors=SF, level_sigma2=(SF * SF).astype(np.float32),
              inv_level_sigma2=(np.float32(1.0) / (SF * SF)).astype(np.float32), log_scale_factor=float(np.log(np.float32(1.2))))


def putable(kf):
    return dict(kf, **LEVELS)


class World:
    """A keyframe store, two map stores, and the bookkeeping that turns a scene's keyframe into (slot, map store, mp_slots) plus the
    keyframe dict the uploaded call must see: mp = mp_slot, bad = the record's bad."""

    def __init__(self, capi):
        self.capi = capi
        self.kfs = capi.KeyframeStore(CAPACITY, SLOT_KEYPOINTS)
        self.maps = [capi.MapStore(POINTS), capi.MapStore(POINTS)]
        self.next = [0, 0]

    def close(self):
        self.kfs.close()
        for m in self.maps:
            m.close()

    def points(self, kf, which=0):
        """The keyframe's map points written to fresh slots of map store `which`; returns (mp_slots, the uploaded call's dict)."""
        has = kf["mp"] >= 0
        k = int(has.sum())
        mp = np.full(len(kf["mp"]), -1, np.int32)
        mp[has] = self.next[which] + np.arange(k, dtype=np.int32)
        self.next[which] += k
        rec = np.zeros(k, self.capi.LOCAL_POINT_DTYPE)
        rec["bad"] = kf["bad"][has]; rec["n_obs"] = 1
        if k:
            self.maps[which].update(mp[has], rec)
        return mp, dict(kf, mp=mp)

    def place(self, kfs, slots, which=None):
        """put kfs to slots, their points to the map stores `which` (default: store 0).  Returns (resident tuples, uploaded dicts)."""
        self.kfs.put(slots, [putable(kf) for kf in kfs])
        self.next = [0, 0]                      # (the map stores' slots are written again from the start)
        res, up = [], []
        for i, kf in enumerate(kfs):
            w = 0 if which is None else which[i]
            mp, u = self.points(kf, w)
            res.append((int(slots[i]), self.maps[w], mp)); up.append(u)
        return res, up


@pytest.fixture(scope="module")
def world(capi):
    w = World(capi)
    yield w
    w.close()


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.BowTargets()
    h.reserve(SLOT_KEYPOINTS, 12, 12 * 450 + 4 * SLOT_KEYPOINTS)
    yield h
    h.close()


def same(h, world, res, up, nnratio=0.9, check_ori=True):
    """uploaded == resident on cur = keyframe 0 against the others; returns the rows"""
    ri, rn = h.search(up[0], up[1:], nnratio, check_ori)
    gi, gn = h.search_resident(world.kfs, res[0], res[1:], nnratio, check_ori)
    assert np.array_equal(gn, rn), (gn, rn)
    assert np.array_equal(gi, ri)
    return gi, gn


def both(h, world, cur, targets, slots=None, **kw):
    kfs = [cur] + list(targets)
    slots = np.arange(len(kfs), dtype=np.int32) if slots is None else np.asarray(slots, np.int32)
    res, up = world.place(kfs, slots)
    return same(h, world, res, up, **kw)


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("dup", [0.0, 0.3])
@pytest.mark.parametrize("T", [1, 3, 11])
def test_parity_grid(chain, world, T, dup, check_ori):
    sc = bts.scene(0, T, dup=dup)
    idx, nm = both(chain, world, sc["cur"], sc["targets"], check_ori=check_ori)
    assert nm.min() > 0 and (idx >= 0).sum() == nm.sum()


@pytest.mark.parametrize("k", [63, 64, 65, 129])
def test_edge_scene(chain, world, k):
    sc = bts.edge_scene(k)
    both(chain, world, sc["cur"], sc["targets"])


def test_boundary_scene(chain, world):
    sc = bts.boundary_scene()
    idx, nm = both(chain, world, sc["cur"], sc["targets"])
    assert (idx[:, 0] == -1).all() and (idx[:, 1] >= 0).all()       # distance 50 stays unmatched, 49 matches


def sized_kf(n, seed):
    """n keypoints out of one pool of SLOT_KEYPOINTS world points: any two such keyframes share their first min(n, n') points."""
    rng = np.random.default_rng(31)
    base = rng.integers(0, 256, (SLOT_KEYPOINTS, 32), dtype=np.uint8)
    node = rng.integers(1, 30, SLOT_KEYPOINTS) * 5 + 1
    ang = rng.uniform(0, 360, SLOT_KEYPOINTS)
    r2 = np.random.default_rng([seed, n])
    d = base[:n].copy()
    d[np.arange(n), r2.integers(0, 32, n)] ^= np.uint8(1) << r2.integers(0, 8, n).astype(np.uint8)
    mp = np.where(r2.random(n) < 0.8, 10 + np.arange(n), -1)
    bad = ((mp >= 0) & (r2.random(n) < 0.1)).astype(np.uint8)
    return bts.make_kf(d, node[:n], mp, bad, np.mod(ang[:n] + 20.0 * seed, 360.0), r2)


@pytest.mark.parametrize("n", [0, 1, WG_THREADS - 1, WG_THREADS, WG_THREADS + 1, WG_SPAN - 1, WG_SPAN, WG_SPAN + 1, SLOT_KEYPOINTS])
def test_prologue_keyframe_sizes(chain, world, n):
    """a keyframe of n keypoints as a target of a full one and as cur against a full one and a small one"""
    full, small, kf = sized_kf(SLOT_KEYPOINTS, 1), sized_kf(300, 2), sized_kf(n, 3)
    idx, nm = both(chain, world, full, [kf, small])
    assert nm[0] > 0 or n < 2
    idx, nm = both(chain, world, kf, [full, small])
    assert idx.shape == (2, n) and (nm[0] > 0 or n < 2)


def test_prologue_no_feature_vector(chain, world):
    sc = bts.scene(0, 3)
    bare = dict(sc["targets"][0], fv=dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(0, np.int32), fv_feat=np.zeros(0, np.int32)))
    idx, nm = both(chain, world, sc["cur"], [bare, sc["targets"][1]])
    assert nm[0] == 0 and (idx[0] == -1).all() and nm[1] > 0
    idx, nm = both(chain, world, bare, sc["targets"][1:])
    assert (nm == 0).all() and (idx == -1).all()


def test_prologue_no_points_and_all_bad(chain, world):
    sc = bts.scene(0, 3)
    tg = [bts.without_map_points(sc["targets"][0]), bts.all_bad(sc["targets"][1]), sc["targets"][2]]
    idx, nm = both(chain, world, sc["cur"], tg)
    assert nm[0] == 0 and nm[1] == 0 and nm[2] > 0
    idx, nm = both(chain, world, bts.all_bad(sc["cur"]), sc["targets"])
    assert (nm == 0).all() and (idx == -1).all()
    # no point anywhere: points may be NULL
    kfs = [bts.without_map_points(k) for k in [sc["cur"]] + sc["targets"][:2]]
    res, up = world.place(kfs, np.arange(3, dtype=np.int32))
    res = [(s, None, mp) for s, _, mp in res]
    idx, nm = same(chain, world, res, up)
    assert (nm == 0).all()


def test_unlisted_features_of_cur_hold_no_match(chain, world):
    """Features of cur that no node lists (stopped words): the prologue's -1 stays in their rows; the resident call has no host pass."""
    sc = bts.scene(0, 3)
    ref, _ = both(chain, world, sc["cur"], sc["targets"])
    hit = np.flatnonzero((ref >= 0).all(axis=0))[:7]
    assert len(hit) == 7
    cur = bts.drop_features(sc["cur"], hit)
    idx, nm = both(chain, world, cur, sc["targets"])
    assert (idx[:, hit] == -1).all() and nm.min() > 0


def test_slots_descending_with_gaps(chain, world):
    sc = bts.scene(0, 3)
    both(chain, world, sc["cur"], sc["targets"], slots=[13, 9, 6, 2])


def test_one_slot_as_cur_and_target_and_twice_under_two_lists(chain, world):
    sc = bts.scene(0, 3)
    res, up = world.place([sc["cur"], sc["targets"][0]], np.array([4, 5], np.int32))
    # cur's own slot as a target; target 0's slot twice, the second time with every other point taken away
    mp2 = res[1][2].copy(); mp2[::2] = -1
    r = [res[0], res[0], res[1], (res[1][0], res[1][1], mp2)]
    u = [up[0], up[0], up[1], dict(up[1], mp=mp2)]
    idx, nm = same(chain, world, r, u)
    assert nm[0] > nm[1] > nm[2] > 0


def test_targets_in_a_second_map_store(chain, world):
    sc = bts.scene(0, 3)
    kfs = [sc["cur"]] + sc["targets"]
    res, up = world.place(kfs, np.arange(4, dtype=np.int32), which=[0, 1, 0, 1])
    assert res[1][1] is world.maps[1] and res[2][1] is world.maps[0]
    _, nm = same(chain, world, res, up)
    assert nm.min() > 0


def test_ordering_against_update_and_put(capi, chain, world):
    """search -> MapStore.update setting points bad -> search -> put of another keyframe to a target's slot -> search, nothing
    synchronising in between: each resident search equals the uploaded call on the state at its time."""
    sc = bts.scene(0, 3)
    other = bts.scene(1, 3)["targets"][2]
    kfs = [sc["cur"]] + sc["targets"]
    res, up = world.place(kfs, np.arange(4, dtype=np.int32))
    run = chain.prepare_resident(world.kfs, res[0], res[1:])
    a = [x.copy() for x in run()]
    # 1. some of target 0's points go bad
    mp0 = res[1][2]
    hit = mp0[(mp0 >= 0) & (up[1]["bad"] == 0)][::2]
    rec = np.zeros(len(hit), capi.LOCAL_POINT_DTYPE); rec["bad"] = 1; rec["n_obs"] = 1
    world.maps[0].update(hit, rec)
    b = [x.copy() for x in run()]
    # 2. another keyframe takes target 1's slot (same size or not: its own mp_slot list)
    world.kfs.put(np.array([2], np.int32), [putable(other)])
    mp_o, up_o = world.points(other)
    c = [x.copy() for x in chain.search_resident(world.kfs, res[0], [res[1], (2, world.maps[0], mp_o), res[3]])]
    bad1 = up[1]["bad"].copy(); bad1[np.isin(mp0, hit)] = 1
    up1 = dict(up[1], bad=bad1)
    for got, tg in ((a, up[1:]), (b, [up1, up[2], up[3]]), (c, [up1, up_o, up[3]])):
        ri, rn = chain.search(up[0], tg)
        assert np.array_equal(got[1], rn) and np.array_equal(got[0], ri)
    assert b[1][0] < a[1][0] and not np.array_equal(c[0][1], b[0][1])


def upload_formula(ns):
    """include/dvmslam_hip.h, dvm_search_by_bow_targets_resident: ns = the keypoints of cur and of every target"""
    r64 = lambda b: (b + 63) // 64 * 64  # noqa: E731
    return r64(56 * len(ns)) + r64(32 * len(ns)) + sum(r64(4 * n) for n in ns)


def test_upload_counter(chain, world):
    sc = bts.scene(0, 11)
    kfs = [sc["cur"]] + sc["targets"]
    res, up = world.place(kfs, np.arange(12, dtype=np.int32))
    chain.search(up[0], up[1:])
    uploaded = chain.last_upload_bytes()
    chain.search_resident(world.kfs, res[0], res[1:])
    resident = chain.last_upload_bytes()
    ns = [len(k["kps"]) for k in kfs]
    assert resident == upload_formula(ns)
    assert resident <= sum((4 * n + 63) // 64 * 64 for n in ns) + 256 * len(ns)
    # the uploaded call: angle, descriptor and flag of every keypoint (37 B) and the FeatureVector; the resident one: 4 B
    assert uploaded >= 37 * sum(ns) and resident * 8 < uploaded, (uploaded, resident)
    # a call that does not reach the device leaves the counter alone
    chain.search_resident(world.kfs, res[0], [])
    assert chain.last_upload_bytes() == resident


def test_refusals_leave_the_handle_usable(capi, chain, world):
    sc = bts.scene(0, 3)
    kfs = [sc["cur"]] + sc["targets"]
    res, up = world.place(kfs, np.arange(4, dtype=np.int32))
    world.kfs.put(np.array([10], np.int32), [putable(sc["cur"])])
    world.kfs.remove(np.array([10], np.int32))
    mp = res[1][2]
    first = int(np.flatnonzero(mp >= 0)[0])

    def with_slot(v):
        m = mp.copy(); m[first] = v
        return (res[1][0], res[1][1], m)
    # a FeatureVector that lists feature f twice (and leaves another out): put takes it, the search does not
    fv = sc["targets"][2]["fv"]
    feat = fv["fv_feat"].copy(); feat[-1] = feat[0]
    twice = dict(sc["targets"][2], fv=dict(fv, fv_feat=feat))
    assert fv["fv_off"][1] < len(feat) - 1      # (two different nodes)
    world.kfs.put(np.array([11], np.int32), [putable(twice)])
    assert np.array_equal(world.kfs.read(11)["fv_feat"], feat)
    with pytest.raises(capi.DvmError) as e:
        chain.search(up[0], [dict(up[3], fv=twice["fv"])])
    assert e.value.code == INVALID
    cases = [
        ("slot outside the store", INVALID, res[0], [(CAPACITY, res[1][1], mp)]),
        ("negative slot", INVALID, res[0], [(-1, res[1][1], mp)]),
        ("slot never written", INVALID, res[0], [(15, res[1][1], mp)]),
        ("slot removed", INVALID, res[0], [(10, res[1][1], res[0][2])]),
        ("removed slot as cur", INVALID, (10, res[0][1], res[0][2]), [res[1]]),
        ("mp_slot outside its map store", INVALID, res[0], [with_slot(POINTS)]),
        ("mp_slot never written", INVALID, res[0], [with_slot(POINTS - 1)]),
        ("mp_slot below -1", INVALID, res[0], [with_slot(-2)]),
        ("NULL mp_slot", INVALID, res[0], [(res[1][0], res[1][1], None)]),
        ("NULL points with a point named", INVALID, res[0], [(res[1][0], None, mp)]),
        ("feature listed twice", INVALID, res[0], [res[1], (11, res[3][1], res[3][2])]),
        ("too many targets", CAPACITY_ERR, res[0], [res[1]] * 13),
    ]
    if capi.device_count() > 1:
        far_kfs, far_map = capi.KeyframeStore(2, 64, device=1), capi.MapStore(POINTS, device=1)
        rec = np.zeros(1, capi.LOCAL_POINT_DTYPE)
        far_map.update(mp[mp >= 0], np.repeat(rec, int((mp >= 0).sum())))
        cases.append(("map store on another device", INVALID, res[0], [(res[1][0], far_map, mp)]))
    for what, code, cur, targets in cases:
        with pytest.raises(capi.DvmError) as e:
            chain.search_resident(world.kfs, cur, targets)
        assert e.value.code == code, what
        same(chain, world, res, up)
    if capi.device_count() > 1:
        with pytest.raises(capi.DvmError) as e:
            chain.search_resident(far_kfs, res[0], res[1:])
        assert e.value.code == INVALID
        same(chain, world, res, up)
        far_kfs.close(); far_map.close()
        capi.MapStore(1, device=0).close()          # (the calling thread's current device is 0 again)
    # beyond the reserved keypoints of cur
    small = capi.BowTargets()
    small.reserve(100, 4, 4 * 450)
    with pytest.raises(capi.DvmError) as e:
        small.search_resident(world.kfs, res[0], res[1:])
    assert e.value.code == CAPACITY_ERR
    small.reserve(450, 4, 4 * 450)
    same(small, world, res, up)
    small.close()
    # legal: no target at all
    idx, nm = chain.search_resident(world.kfs, res[0], [])
    assert idx.shape == (0, len(res[0][2])) and len(nm) == 0
