"""dvm_fuse_targets_run_hits_candidates: the second direction of SearchInNeighbors.  cand_slot against the numpy restatement of
vpFuseCandidates (fuse_points_scene.candidates), the hits against dvm_fuse_targets_run_hits_resident on that list with the exclude mask:
one and three lists, totals around the wave, the block and the compaction rounds, duplicates inside and across lists, nothing but -1,
nothing but bad points, exclude absent / given / with -1 entries, one and three targets; the tables idle again after a call and after a
refused call; the capacities."""
import numpy as np
import pytest

import fuse_points_scene as fps
import fuse_targets_scene as fts

pytestmark = pytest.mark.gpu

N_CLOUD = 300
MAX_ENTRIES = 1100
INVALID, CAPACITY = -1, -3


@pytest.fixture(scope="module")
def world(capi):
    """the scene's points in a map store (every fifth bad), a chain per target count"""
    sc = fts.scene(2, 3, N_CLOUD)
    bad = (np.arange(N_CLOUD) % 5 == 4).astype(np.int32)
    store = capi.MapStore(3 * N_CLOUD + 4)
    slots = (store.capacity - 1 - np.cumsum(np.r_[0, 2 + (np.arange(N_CLOUD - 1) % 2)])).astype(np.int32)
    store.update(slots, fps.records(sc["pts"], bad))
    bad_of_slot = np.zeros(store.capacity, bool); bad_of_slot[slots] = bad != 0
    chains = {}
    for T in (1, 3):
        h = capi.FuseTargets()
        h.reserve(MAX_ENTRIES, 3, sum(len(kf["kps"]) for kf in sc["targets"]))
        h.reserve_hits(3 * MAX_ENTRIES)
        h.reserve_candidates(MAX_ENTRIES, store.capacity)
        h.set(sc["targets"][:T])
        chains[T] = h
    yield dict(sc=sc, store=store, slots=slots, bad=bad_of_slot, chains=chains)
    for h in chains.values():
        h.close()
    store.close()


def make_lists(w, total, n_lists, seed):
    """total entries over n_lists lists: slots of the scene with repeats, -1 entries, a duplicate inside list 0 and one across lists"""
    rng = np.random.default_rng([total, n_lists, seed])
    flat = w["slots"][rng.integers(0, N_CLOUD, total)].astype(np.int32)
    flat[rng.random(total) < 0.15] = -1
    cuts = np.sort(rng.integers(0, total + 1, n_lists - 1)) if total >= 8 else np.zeros(n_lists - 1, int)
    if total >= 8:
        good = w["slots"][np.flatnonzero(~w["bad"][w["slots"]])]
        flat[0] = good[0]; flat[2] = good[0]                                 # inside the first list (its first cut lies behind)
        cuts = np.maximum(cuts, 3)
        flat[total - 1] = good[0]; flat[1] = good[1]; flat[total - 2] = good[1]
    return [a.copy() for a in np.split(flat, cuts)]


def check(w, T, lists, exclude=None):
    h, store = w["chains"][T], w["store"]
    cand, off, hits = h.run_hits_candidates(store, lists, 3.0, exclude)
    want = fps.candidates(lists, w["bad"])
    assert np.array_equal(cand, want)
    ex = np.zeros(0, np.int32) if exclude is None else np.asarray(exclude, np.int32)
    skip = np.tile(np.isin(want, ex[ex >= 0]).astype(np.uint8), (T, 1))
    woff, whits = h.run_hits_resident(store, want, 3.0, skip)
    assert np.array_equal(off, woff) and np.array_equal(hits, whits)
    return cand, off, hits


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n_lists", [1, 3])
@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_lists(world, total, n_lists, T):
    lists = make_lists(world, total, n_lists, 0)
    assert sum(len(a) for a in lists) == total and len(lists) == n_lists
    if total >= 8:                                                           # the first occurrence wins: as constructed
        flat = np.concatenate(lists)
        assert flat[0] == flat[2] == flat[-1] and flat[1] == flat[-2] and len(lists[0]) >= 3
    cand, off, hits = check(world, T, lists)
    if total >= 8:
        assert cand[0] == lists[0][0] and cand[1] == lists[0][1] and (cand == cand[0]).sum() == 1
    ex = np.concatenate([cand[::3], [-1, -1]]).astype(np.int32)             # exclude given, holding -1 entries
    c2, off2, hits2 = check(world, T, lists, ex)
    assert np.array_equal(c2, cand)
    if total == 1025:
        assert off[-1] >= 5 and 0 < off2[-1] < off[-1]
        assert not np.isin(cand[hits2["point"]], ex).any()


def test_nothing_to_list(world):
    w = world
    bad_slots = w["slots"][np.flatnonzero(w["bad"][w["slots"]])]
    for lists in ([np.full(70, -1, np.int32)], [bad_slots[:40], bad_slots[:3]], [np.zeros(0, np.int32)], []):
        cand, off, hits = check(w, 3, lists, exclude=w["slots"][:5])
        assert len(cand) == 0 and (off == 0).all() and len(hits) == 0
    cand, off, hits = w["chains"][1].run_hits_candidates(None, [np.full(9, -1, np.int32)])      # no store: no point named
    assert len(cand) == 0 and (off == 0).all()


def test_no_targets(world, capi):
    """T = 0: the list is still made, there is nothing to search"""
    w = world
    h = capi.FuseTargets()
    h.reserve(MAX_ENTRIES, 1, 4096); h.reserve_hits(16); h.reserve_candidates(MAX_ENTRIES, w["store"].capacity)
    h.set(w["sc"]["targets"][:1]); h.set([])                                 # (an earlier set with targets leaves nothing to search either)
    lists = make_lists(w, 257, 3, 2)
    for _ in range(2):
        cand, off, hits = h.run_hits_candidates(w["store"], lists, 3.0, exclude=lists[0])
        assert np.array_equal(cand, fps.candidates(lists, w["bad"])) and list(off) == [0] and len(hits) == 0
    bi, bd = h.run_resident(w["store"], cand, 3.0)
    assert bi.shape == (0, len(cand))
    h.close()


def test_tables_are_idle_again(world, capi):
    w = world
    h = w["chains"][3]
    good = w["slots"][np.flatnonzero(~w["bad"][w["slots"]])]
    base = h.run_hits_resident(w["store"], good, 3.0)
    hit_pts = np.unique(base[1]["point"])
    assert len(hit_pts) >= 4
    s, e = good[hit_pts[0]], good[hit_pts[1]]
    others = good[hit_pts[2:4]]
    A = [np.array([s, e, others[0], -1, others[1]], np.int32)]               # s first at flat index 0; e excluded
    B = [np.array([others[0], e, others[1], s, s], np.int32)]                # s first at index 3; nothing excluded
    ca, offa, hitsa = check(w, 3, A, exclude=[e])
    assert not (ca[hitsa["point"]] == e).any() and (ca[hitsa["point"]] == s).any()
    cb, offb, hitsb = check(w, 3, B)
    assert list(cb) == [others[0], e, others[1], s]                          # B lists s ...
    assert (cb[hitsb["point"]] == e).any()                                   # ... and searches e
    # the same behind a refused call (a slot never written inside A: nothing is queued)
    refused = [np.array([s, e, int(w["slots"][0]) - 1], np.int32)]
    with pytest.raises(capi.DvmError) as err:
        h.run_hits_candidates(w["store"], refused, 3.0, [e])
    assert err.value.code == INVALID and err.value.n_cand == -7 and (err.value.hit_off == -7).all()
    cb2, offb2, hitsb2 = check(w, 3, B)
    assert np.array_equal(cb2, cb) and np.array_equal(hitsb2, hitsb)
    # and behind a call that ran out of cand_cap (its kernels ran)
    with pytest.raises(capi.DvmError):
        h.run_hits_candidates(w["store"], A, 3.0, [e], cand_cap=2)
    cb3, _, hitsb3 = check(w, 3, B)
    assert np.array_equal(cb3, cb) and np.array_equal(hitsb3, hitsb)


def test_capacities(world, capi):
    w = world
    h = w["chains"][1]
    lists = make_lists(w, 257, 3, 1)
    want = fps.candidates(lists, w["bad"])
    n = len(want)
    assert n > 64
    with pytest.raises(capi.DvmError) as e:
        h.run_hits_candidates(w["store"], lists, 3.0, cand_cap=n - 1, guard=8)
    assert e.value.code == CAPACITY and e.value.n_cand == n and (e.value.cand_tail == -7).all()
    cand, off, hits = check(w, 1, lists)                                     # the next call is good
    assert len(cand) == n
    cand, _, _ = h.run_hits_candidates(w["store"], lists, 3.0, cand_cap=n)  # exactly the count fits
    assert np.array_equal(cand, want)
    too_long = [w["slots"][np.arange(MAX_ENTRIES + 1) % N_CLOUD]]
    with pytest.raises(capi.DvmError) as e:
        h.run_hits_candidates(w["store"], too_long, 3.0)
    assert e.value.code == CAPACITY and e.value.n_cand == -7
    small = capi.FuseTargets()
    small.reserve(100, 1, 4096); small.reserve_hits(300)
    small.set(w["sc"]["targets"][:1])
    with pytest.raises(capi.DvmError) as e:                                  # before reserve_candidates
        small.run_hits_candidates(w["store"], lists, 3.0)
    assert e.value.code == INVALID and "reserve_candidates" in str(e.value)
    small.reserve_candidates(400, 8)
    with pytest.raises(capi.DvmError) as e:                                  # the bound beyond max_points
        small.run_hits_candidates(w["store"], lists, 3.0)
    assert e.value.code == CAPACITY and "max_points" in str(e.value)
    small.reserve(300, 1, 4096); small.set(w["sc"]["targets"][:1])
    with pytest.raises(capi.DvmError) as e:                                  # a store of more slots than map_capacity
        small.run_hits_candidates(w["store"], lists, 3.0)
    assert e.value.code == CAPACITY and "map_capacity" in str(e.value)
    small.reserve_candidates(200, w["store"].capacity)                      # (grow-only: max_entries stays 400)
    got = small.run_hits_candidates(w["store"], lists, 3.0)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], off) and np.array_equal(got[2], hits)
    small.close()
    tiny = capi.FuseTargets()
    tiny.reserve(300, 1, 4096); tiny.reserve_hits(300); tiny.set(w["sc"]["targets"][:1])
    tiny.reserve_candidates(200, w["store"].capacity)
    with pytest.raises(capi.DvmError) as e:                                  # the bound beyond max_entries
        tiny.run_hits_candidates(w["store"], lists, 3.0)
    assert e.value.code == CAPACITY and "max_entries" in str(e.value)
    tiny.close()
