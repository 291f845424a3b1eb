"""dvm_fuse_targets_run_hits (the hits of a run instead of its dense rows), dvmh_fuse_sim3_targets + dvmh_fuse_sim3_apply
(LoopClosing::SearchAndFuse as one chain) and their refusals.  The hits must be exactly the entries with best_idx >= 0 of
dvm_fuse_targets_run on the same inputs, target by target in ascending point; hit counts are shaped by masking the surplus hits of the dense
rows, so that the wave tail (63, 64, 65) and the round tail (255, 256, 257) of the compaction are met exactly."""
import numpy as np
import pytest

import fuse_cam_scene as fcs
import fuse_targets_scene as fts
import kb8_scene as ks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.FuseTargets()
    h.reserve(900, 33, 33 * 300 + 2000)
    h.reserve_hits(33 * 900)
    yield h
    h.close()


def _chain_pts(pts, use_valid=True):
    return {k: v for k, v in pts.items() if k in ("pos", "normal", "min_dist", "max_dist", "desc") or (use_valid and k == "valid")}


def _same_hits(chain, pts, th, skip):
    """run and run_hits on the same inputs; returns (best_idx, hit_off, hits)."""
    bi, bd = chain.run(pts, th, skip)
    off, hits = chain.run_hits(pts, th, skip)
    want_off, want = fcs.hits_of(bi, bd)
    assert np.array_equal(off, want_off) and hits.dtype == want.dtype and hits.tobytes() == want.tobytes()
    return bi, off, hits


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 200])
@pytest.mark.parametrize("T", [1, 2, 5, 33])
def test_hits_are_the_hits_of_run_pinhole(chain, T, n, form):
    sc = fcs.scw_scene(T)
    pts = _chain_pts({k: v[:n] for k, v in sc["pts"].items()})
    chain.set([fcs.chain_target(kf) for kf in sc["targets"]], forms=[form] * T)
    for skip in (None, sc["skip"][:, :n]):
        bi, off, hits = _same_hits(chain, pts, fcs.TH, skip)
    if n == 200:
        bi, off, hits = _same_hits(chain, pts, fcs.TH, None)
        assert off[-1] == len(hits) >= 20 * T


@pytest.mark.parametrize("model", list(ks.MODELS))
def test_hits_are_the_hits_of_run_kb8_and_mixed(capi, chain, model):
    sc = fcs.kb8_scene(model, 5, 900)
    tg = [fcs.kb8_chain_target(x) for x in sc["targets"]]
    kb8, pin = capi.CameraModel.make(1, ks.MODELS[model]), capi.CameraModel.pinhole(*ks.PINHOLE_WIDE[:4])
    for models, forms in (([kb8] * 5, [0] * 5), ([kb8] * 5, [1] * 5), ([kb8, pin, kb8, pin, pin], [0, 1, 1, 0, 1])):
        chain.set(tg, models=models, forms=forms)
        bi, off, hits = _same_hits(chain, _chain_pts(sc["pts"]), fcs.KB8_TH, sc["skip"])
        assert off[fcs.KB8_EMPTY_TARGET] == off[fcs.KB8_EMPTY_TARGET + 1] and len(hits) > 500


def _shape_counts(bi, counts):
    """A mask [T, n] that leaves target t exactly counts[t] of its hits (the first ones) and every miss."""
    mask = np.zeros(bi.shape, np.uint8)
    for t, c in enumerate(counts):
        h = np.flatnonzero(bi[t] >= 0)
        assert len(h) >= c, (t, len(h), c)
        mask[t, h[c:]] = 1
    return mask


def test_wave_and_round_tails(chain):
    """Per-target hit counts of exactly 0, 1, 63, 64, 65 and, in one target, 255, 256, 257."""
    sc = fcs.scw_scene(33, 700, n_cloud=700)
    T = 33
    pts = _chain_pts(sc["pts"], False)
    chain.set([fcs.chain_target(kf) for kf in sc["targets"]], forms=[1] * T)
    bi, bd = chain.run(pts, fcs.TH)
    have = (bi >= 0).sum(axis=1)
    big = int(np.argmax(have))
    assert have[big] >= 257, have
    rich = [t for t in np.argsort(-have) if t != big][:5]
    assert have[rich[-1]] >= 65, have
    for big_count in (255, 256, 257):
        counts = np.minimum(have, 3)
        counts[big] = big_count
        for t, c in zip(rich, (0, 1, 63, 64, 65)):
            counts[t] = c
        mask = _shape_counts(bi, counts)
        off, hits = chain.run_hits(pts, fcs.TH, mask)
        assert np.array_equal(np.diff(off), counts)
        want_off, want = fcs.hits_of(np.where(mask != 0, -1, bi), bd)
        assert np.array_equal(off, want_off) and hits.tobytes() == want.tobytes()


def test_empty_target_between_full_ones_and_all_masked(chain):
    sc = fcs.scw_scene(5)
    pts = _chain_pts(sc["pts"])
    chain.set([fcs.chain_target(kf) for kf in sc["targets"]], forms=[1] * 5)
    bi, off, hits = _same_hits(chain, pts, fcs.TH, None)
    e = fts.EMPTY_TARGET
    assert off[e] == off[e + 1] and off[e] > 50 and off[e + 2] - off[e + 1] > 50        # hit_off repeats between two full targets
    off, hits = chain.run_hits(pts, fcs.TH, np.ones((5, 200), np.uint8))               # all entries masked
    assert np.all(off == 0) and len(hits) == 0
    chain.set([])                                                                       # T = 0
    off, hits = chain.run_hits(pts, fcs.TH)
    assert list(off) == [0] and len(hits) == 0
    chain.set([fcs.chain_target(kf) for kf in sc["targets"]], forms=[1] * 5)
    off, hits = chain.run_hits({k: v[:0] for k, v in pts.items()}, fcs.TH)            # n = 0
    assert list(off) == [0] * 6 and len(hits) == 0


def test_capacity_one_short(capi, chain):
    sc = fcs.scw_scene(33)
    pts = _chain_pts(sc["pts"])
    chain.set([fcs.chain_target(kf) for kf in sc["targets"]], forms=[1] * 33)
    bi, off, hits = _same_hits(chain, pts, fcs.TH, sc["skip"])
    total = len(hits)
    assert total > 1000
    with pytest.raises(capi.DvmError) as e:
        chain.run_hits(pts, fcs.TH, sc["skip"], hit_cap=total - 1, guard=64)
    assert e.value.code == -3 and e.value.n_hits == total and np.array_equal(e.value.hit_off, off)      # the full counts
    assert np.all(e.value.tail.view(np.int32) == -7)                                                    # nothing behind hits[hit_cap]
    off2, hits2 = chain.run_hits(pts, fcs.TH, sc["skip"], hit_cap=total, guard=64)                     # a repeat with room
    assert np.array_equal(off2, off) and hits2.tobytes() == hits.tobytes()
    # beyond the reservation: the same answer, and the handle stays usable
    h = capi.FuseTargets()
    h.reserve(200, 33, 33 * 300 + 2000)
    h.reserve_hits(total - 1)
    h.set([fcs.chain_target(kf) for kf in sc["targets"]], forms=[1] * 33)
    with pytest.raises(capi.DvmError) as e:
        h.run_hits(pts, fcs.TH, sc["skip"])
    assert e.value.code == -3 and e.value.n_hits == total and np.array_equal(e.value.hit_off, off)
    h.reserve_hits(total)
    off3, hits3 = h.run_hits(pts, fcs.TH, sc["skip"])
    assert np.array_equal(off3, off) and hits3.tobytes() == hits.tobytes()
    h.close()


def test_run_twice_the_same_bytes(chain):
    sc = fcs.scw_scene(33)
    pts = _chain_pts(sc["pts"])
    chain.set([fcs.chain_target(kf) for kf in sc["targets"]], forms=np.arange(33) % 2)
    a = chain.run_hits(pts, fcs.TH, sc["skip"])
    b = chain.run_hits(pts, fcs.TH, sc["skip"])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[1]) > 1000


@pytest.mark.parametrize("T", [5, 33])
def test_search_and_fuse_against_the_loop_of_fuse_sim3(capi, T):
    """The loop of dvmh_fuse_sim3 over the keyframes (on copies) against dvmh_fuse_sim3_targets + dvmh_fuse_sim3_apply: replace, nFused and
    every keyframe's mvpMapPoints identical."""
    sc = fcs.scw_scene(T)
    pts = sc["pts"]
    P = capi.map_points_view(pts)
    loop = []
    for kf in sc["targets"]:
        d = dict(kf, mp=kf["mp"].copy())
        n, rep = capi.fuse_sim3(capi.keyframe_view(d), kf["Scw"], P, fcs.TH)
        loop.append((n, rep.copy(), d["mp"]))
    kfs = [dict(kf, mp=kf["mp"].copy()) for kf in sc["targets"]]
    views = [capi.keyframe_view(d) for d in kfs]
    Scws = np.stack([kf["Scw"] for kf in sc["targets"]])
    off, hits = capi.fuse_sim3_targets(views, Scws, P, fcs.TH)
    want_off, want = fcs.hits_of(*fcs.scw_rows(sc["targets"], pts, fcs.already_found_mask(sc["targets"], pts)))
    assert np.array_equal(off, want_off) and hits.tobytes() == want.tobytes()          # ... and the oracle's ungated rows
    with pytest.raises(capi.DvmError) as e:                                             # hit_cap one short: the counts come back
        capi.fuse_sim3_targets(views, Scws, P, fcs.TH, hit_cap=len(hits) - 1)
    assert e.value.code == -3 and np.array_equal(e.value.hit_off, off)
    off2, hits2 = capi.fuse_sim3_targets(views, Scws, P, fcs.TH, hit_cap=len(hits))     # ... and size the repeat
    assert np.array_equal(off2, off) and hits2.tobytes() == hits.tobytes()
    fused = 0
    for t in range(T):
        n, rep = capi.fuse_sim3_apply(views[t], P, hits[off[t]:off[t + 1]])
        assert n == loop[t][0] and np.array_equal(rep, loop[t][1]) and np.array_equal(kfs[t]["mp"], loop[t][2]), t
        fused += n
    assert fused >= 20 * T


def test_stale_rows_are_refreshed_by_masked_runs_in_the_scw_form(chain):
    """tests/test_gpu_fuse_targets.py's refresh in form 1 through run_hits: descriptors of a few points change after targets 1 and 3 of 5;
    one speculative run, then one masked run per boundary over (stale points) x (later targets) assembles the hits of the sequential loop."""
    sc = fcs.scw_scene(5)
    rng = np.random.default_rng(5)
    pts = {k: v.copy() for k, v in _chain_pts(sc["pts"]).items()}
    donors = fts.scene(1, 33)["pts"]["desc"]
    changes = {1: rng.choice(200, 9, replace=False), 3: rng.choice(200, 7, replace=False)}
    base_skip = ((sc["skip"] != 0) | (pts["valid"][None, :] == 0)).astype(np.uint8)
    want_i = np.zeros((5, 200), np.int32); want_d = np.zeros((5, 200), np.int32)
    cur = {k: v.copy() for k, v in pts.items()}
    for t in range(5):
        i, d = fcs.scw_rows(sc["targets"][t:t + 1], cur, base_skip[t:t + 1])
        want_i[t], want_d[t] = i[0], d[0]
        if t in changes:
            cur["desc"][changes[t]] = donors[changes[t]]
    chain.set([fcs.chain_target(kf) for kf in sc["targets"]], forms=[1] * 5)

    def dense(off, hits):
        bi = np.full((5, 200), -1, np.int32); bd = np.full((5, 200), 256, np.int32)
        for t in range(5):
            h = hits[off[t]:off[t + 1]]
            bi[t, h["point"]] = h["idx"]; bd[t, h["point"]] = h["dist"]
        return bi, bd
    got_i, got_d = dense(*chain.run_hits(pts, fcs.TH, sc["skip"]))
    first_i = got_i.copy()
    stale = np.zeros(200, bool)
    cur = {k: v.copy() for k, v in pts.items()}
    for t in sorted(changes):
        cur["desc"][changes[t]] = donors[changes[t]]
        stale[changes[t]] = True
        let = np.zeros((5, 200), bool); let[t + 1:, stale] = True
        ri, rd = dense(*chain.run_hits(cur, fcs.TH, (~let | (sc["skip"] != 0)).astype(np.uint8)))
        assert np.all(ri[~let] == -1)
        got_i[let] = ri[let]; got_d[let] = rd[let]
    hit = want_i >= 0
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d[hit], want_d[hit])
    assert (first_i != want_i).sum() >= 3                                               # the refresh was needed


def test_run_hits_before_reserve_hits_and_handle_memory(capi):
    import psutil
    import torch

    sc = fcs.scw_scene(5)
    pts = _chain_pts(sc["pts"])
    tg = [fcs.chain_target(kf) for kf in sc["targets"]]
    h = capi.FuseTargets()
    h.reserve(200, 5, 5 * 300 + 2000)
    h.set(tg, forms=[1] * 5)
    want = h.run(pts, fcs.TH, sc["skip"])
    with pytest.raises(capi.DvmError) as e:
        h.run_hits(pts, fcs.TH, sc["skip"])                                            # run_hits before reserve_hits
    assert e.value.code == -1
    got = h.run(pts, fcs.TH, sc["skip"])                                               # ... the resident targets still serve
    assert got[0].tobytes() == want[0].tobytes()
    h.reserve_hits(1000)
    off, hits = h.run_hits(pts, fcs.TH, sc["skip"])
    assert hits.tobytes() == fcs.hits_of(*want)[1].tobytes()
    h.reserve(900, 33, 33 * 2000)                                                      # growing the working set keeps the hit block
    h.set(tg, forms=[1] * 5)
    off2, hits2 = h.run_hits(pts, fcs.TH, sc["skip"])
    assert np.array_equal(off2, off) and hits2.tobytes() == hits.tobytes()
    h.close()

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    def cycle():
        h = capi.FuseTargets()
        h.reserve_hits(500)
        h.reserve(200, 5, 5 * 300 + 2000)
        h.set(tg, forms=[1] * 5); h.run_hits(pts, fcs.TH, sc["skip"])
        h.reserve(900, 33, 33 * 2000)
        h.reserve_hits(33 * 900)
        h.set(tg, forms=[1] * 5); h.run_hits(pts, fcs.TH)
        h.close()
    cycle(); cycle()
    base, rss0 = used(), psutil.Process().memory_info().rss
    for _ in range(50):
        cycle()
    grown = used() - base
    assert grown <= 8 << 20, f"{grown / 2**20:.1f} MiB of device memory not returned after 50 chain handles"
    grown_host = psutil.Process().memory_info().rss - rss0
    assert grown_host <= 96 << 20, f"host memory grew by {grown_host / 2**20:.1f} MiB over 50 chain handles"
