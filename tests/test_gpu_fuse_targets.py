"""dvm_fuse_targets (the Fuse searches of LocalMapping::SearchInNeighbors against all target keyframes as one chain) against
pyoracle.project_search target by target, against the separate HIP calls it batches (capi.fuse, dvm_project_search) and against its own
host entry.  Kernel and oracle run one operation sequence, so best_idx and best_dist are compared exactly.  The scenes are pinned by
tests/test_oracle_fuse_targets.py (CPU)."""
import functools

import numpy as np
import pytest

import fuse_targets_scene as fts

pytestmark = pytest.mark.gpu

SEED_OF_T = {1: 3, 2: 2, 5: 0, 33: 1}          # the pinned scenes


@functools.lru_cache(maxsize=None)
def _oracle(T, n, masked, use_valid):
    sc = fts.prefix(fts.scene(SEED_OF_T[T], T), n)
    return fts.oracle_rows(sc["targets"], sc["pts"], sc["skip"] if masked else None, use_valid)


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.FuseTargets()
    h.reserve(200, 33, 33 * 300 + 2000)
    yield h
    h.close()


def _pts(sc, use_valid):
    return sc["pts"] if use_valid else {k: v for k, v in sc["pts"].items() if k != "valid"}


@pytest.mark.parametrize("masked,use_valid", [(False, False), (True, True), (False, True)], ids=("plain", "masked_valid", "valid"))
@pytest.mark.parametrize("n", [1, 15, 16, 17, 200])
@pytest.mark.parametrize("T", [1, 2, 5, 33])
def test_parity_with_oracle(chain, T, n, masked, use_valid):
    sc = fts.prefix(fts.scene(SEED_OF_T[T], T), n)
    chain.set(sc["targets"])
    bi, bd = chain.run(_pts(sc, use_valid), 3.0, sc["skip"] if masked else None)
    want_i, want_d = _oracle(T, n, masked, use_valid)
    assert np.array_equal(bi, want_i) and np.array_equal(bd, want_d)
    if n == 200:
        assert (bi >= 0).sum() >= 0.25 * T * n * (0.6 if masked else 0.8)


@pytest.mark.parametrize("T", [5, 33])
def test_parity_with_the_separate_calls(capi, chain, T):
    """The chain is a batching of the existing HIP calls, not a new result: capi.fuse per target, dvm_project_search's raw row, the host entry."""
    sc = fts.prefix(fts.scene(SEED_OF_T[T], T), 200)
    pts, skip = sc["pts"], sc["skip"]
    chain.set(sc["targets"])
    bi, bd = chain.run(pts, 3.0, skip)
    P = capi.map_points_view(dict(pts, id=np.arange(200, dtype=np.int32), bad=1 - pts["valid"]))
    views = [capi.keyframe_view(kf) for kf in sc["targets"]]
    total = 0
    for t in (range(T) if T == 5 else (0, 1, 7, 32)):
        kf = sc["targets"][t]
        n_t, row = capi.fuse(views[t], P, skip[t], 3.0)
        assert np.array_equal(row, bi[t]) and n_t == (bi[t] >= 0).sum()
        if len(kf["kps"]):
            g = capi.FrameGrid(2048)
            g.build(kf["kps"], kf["desc"], tuple(float(x) for x in kf["bounds"]))
            cam = dict(Tcw=kf["Tcw"], Ow=capi.se3_inverse(kf["Tcw"])[4:], K=kf["K"], bounds=kf["bounds"], log_scale_factor=kf["log_scale_factor"])
            m, _ = capi.project_search(g, cam, pts, 3.0, kf["scale_factors"], gate_inv_sigma2=kf["inv_level_sigma2"], gate=5.99,
                                       valid=pts["valid"] & (1 - skip[t]))
            g.close()
            assert np.array_equal(m["best_dist"], bd[t]) and np.array_equal(np.where(m["best_dist"] <= 50, m["best_idx"], -1), bi[t])
    total, hbi = capi.fuse_targets(views, P, skip, 3.0)
    assert np.array_equal(hbi, bi) and total == (bi >= 0).sum() > 0.15 * T * 200
    total, hbi = capi.fuse_targets(views, capi.map_points_view(_pts(sc, False)), None, 3.0)     # no id, no bad, no mask
    assert np.array_equal(hbi, _oracle(T, 200, False, False)[0])


def test_stale_rows_are_refreshed_by_masked_runs(chain):
    """The host's role at the data level: descriptors of a few points change after targets 1 and 3 of 5 (what MapPoint::Replace's
    ComputeDistinctiveDescriptors does to a survivor); one speculative run, then one masked run per boundary over (stale points) x
    (later targets), must assemble the rows of the sequential per-target loop with the descriptors current at each target."""
    sc = fts.prefix(fts.scene(0, 5), 200)
    rng = np.random.default_rng(5)
    pts = {k: v.copy() for k, v in sc["pts"].items()}
    donors = fts.scene(1, 33)["pts"]["desc"]
    changes = {1: rng.choice(200, 9, replace=False), 3: rng.choice(200, 7, replace=False)}     # after target t: these points' descriptors
    # the sequential loop, oracle
    want_i = np.zeros((5, 200), np.int32); want_d = np.zeros((5, 200), np.int32)
    cur = {k: v.copy() for k, v in pts.items()}
    for t in range(5):
        i, d = fts.oracle_rows(sc["targets"][t:t + 1], cur, sc["skip"][t:t + 1])
        want_i[t], want_d[t] = i[0], d[0]
        if t in changes:
            cur["desc"][changes[t]] = donors[changes[t]]
    # the chain: one speculative run with the descriptors at entry, then the masked refreshes
    chain.set(sc["targets"])
    first_i, first_d = chain.run(pts, 3.0, sc["skip"])
    got_i, got_d = first_i.copy(), first_d.copy()
    stale = np.zeros(200, bool)
    cur = {k: v.copy() for k, v in pts.items()}
    refreshed = np.zeros((5, 200), bool)
    for t in sorted(changes):
        cur["desc"][changes[t]] = donors[changes[t]]
        stale[changes[t]] = True
        let = np.zeros((5, 200), bool); let[t + 1:, stale] = True
        ri, rd = chain.run(cur, 3.0, (~let | (sc["skip"] != 0)).astype(np.uint8))
        assert np.all(ri[~let] == -1) and np.all(rd[~let] == 256)                     # masked entries read "none"
        got_i[let] = ri[let]; got_d[let] = rd[let]
        refreshed |= let
    assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d)
    assert np.array_equal(got_i[~refreshed], first_i[~refreshed])                    # rows outside the masks stay as the first run left them
    assert (first_d != want_d).sum() >= 5                                            # the refresh was needed


def test_reuse(capi):
    h = capi.FuseTargets()
    h.reserve(200, 33, 33 * 300 + 2000)
    big = fts.prefix(fts.scene(1, 33), 200)
    h.set(big["targets"])
    a = h.run(big["pts"], 3.0, big["skip"])
    b = h.run(big["pts"], 3.0, big["skip"])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()      # run twice: the same bits
    assert np.array_equal(a[0], _oracle(33, 200, True, True)[0])
    small = fts.prefix(fts.scene(2, 2), 17)                                           # a smaller set after a larger one: no rows of the old targets
    h.set(small["targets"])
    i, d = h.run(small["pts"], 3.0, small["skip"])
    assert i.shape == (2, 17) and np.array_equal(i, _oracle(2, 17, True, True)[0]) and np.array_equal(d, _oracle(2, 17, True, True)[1])
    h.set(fts.scene(0, 5)["targets"])                                                 # the same points against new targets
    i, _ = h.run(big["pts"], 3.0, None, want_dist=False)
    assert np.array_equal(i, fts.oracle_rows(fts.scene(0, 5)["targets"], big["pts"])[0])
    h.close()


def test_edges(chain):
    sc = fts.prefix(fts.scene(0, 5), 200)
    chain.set([])                                                                     # T = 0: writes nothing
    i, d = chain.run(sc["pts"], 3.0)
    assert i.shape == (0, 200)
    chain.set(sc["targets"])
    i, d = chain.run(fts.prefix(sc, 0)["pts"], 3.0)                                   # N = 0
    assert i.shape == (5, 0)
    i, d = chain.run(sc["pts"], 3.0, np.ones((5, 200), np.uint8))                     # all masked
    assert np.all(i == -1) and np.all(d == 256)
    i, d = chain.run(_pts(sc, False), 3.0)                                            # the empty target
    assert np.all(i[fts.EMPTY_TARGET] == -1) and np.all(d[fts.EMPTY_TARGET] == 256) and (i[0] >= 0).sum() > 50
    chain.set([sc["targets"][fts.EMPTY_TARGET]])                                      # ... alone
    i, d = chain.run(sc["pts"], 3.0)
    assert np.all(i == -1) and np.all(d == 256)


def test_refusals_leave_the_handle_usable(capi):
    h = capi.FuseTargets()
    sc = fts.prefix(fts.scene(0, 5), 200)
    want = _oracle(5, 200, True, True)

    def code_of(fn):
        with pytest.raises(capi.DvmError) as e:
            fn()
        return e.value.code
    assert code_of(lambda: h.run(sc["pts"], 3.0)) == -1                               # run before set
    assert code_of(lambda: h.set(sc["targets"])) == -3                                # nothing reserved
    h.reserve(200, 5, 5 * 300 + 2000)
    h.set(sc["targets"])

    def refused(code, fn):
        assert code_of(fn) == code
        i, d = h.run(sc["pts"], 3.0, sc["skip"])                                      # ... the resident targets still serve
        assert np.array_equal(i, want[0]) and np.array_equal(d, want[1])
        h.set(sc["targets"])                                                          # ... and so does a good set
        assert np.array_equal(h.run(sc["pts"], 3.0, sc["skip"])[0], want[0])

    def changed(t, **kw):
        tg = list(sc["targets"]); tg[t] = dict(tg[t], **kw)
        return tg
    refused(-3, lambda: h.set(fts.scene(1, 33)["targets"][:6]))                       # more targets than reserved
    refused(-3, lambda: h.set([fts.scene(1, 33)["targets"][-1]] * 3))                 # their keypoints beyond the reservation
    refused(-3, lambda: h.run({k: np.concatenate([v, v]) for k, v in sc["pts"].items()}, 3.0))   # more points than reserved
    n = 8193
    refused(-1, lambda: h.set(changed(2, kps=np.zeros(n, capi.KP_DTYPE), desc=np.zeros((n, 32), np.uint8))))
    refused(-1, lambda: h.set(changed(0, **{k: np.ones(65, np.float32) for k in ("scale_factors", "level_sigma2", "inv_level_sigma2")})))
    refused(-1, lambda: h.set(changed(3, K=np.array([0.0, 500.0, 320.0, 240.0], np.float32))))
    refused(-1, lambda: h.set(changed(3, K=np.array([500.0, 0.0, 320.0, 240.0], np.float32))))
    refused(-1, lambda: h.set(changed(4, inv_level_sigma2=None)))                     # a missing array
    bad_oct = sc["targets"][0]["kps"].copy(); bad_oct["octave"][5] = 8
    refused(-1, lambda: h.set(changed(0, kps=bad_oct)))                               # an octave outside the level tables
    refused(-1, lambda: h.run({k: v for k, v in sc["pts"].items() if k != "valid"} | dict(normal=np.zeros((0, 3), np.float32)), 3.0))
    h.close()


def test_handles_release_their_memory(capi):
    import psutil
    import torch

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free
    sc = fts.prefix(fts.scene(0, 5), 200)

    def cycle():
        h = capi.FuseTargets()
        h.reserve(200, 5, 5 * 300 + 2000)
        h.set(sc["targets"]); h.run(sc["pts"], 3.0, sc["skip"])
        h.reserve(900, 33, 33 * 2000)
        h.set(sc["targets"]); h.run(sc["pts"], 3.0)
        h.close()
    cycle(); cycle()
    base, rss0 = used(), psutil.Process().memory_info().rss
    for _ in range(50):
        cycle()
    grown = used() - base
    assert grown <= 8 << 20, f"{grown / 2**20:.1f} MiB of device memory not returned after 50 chain handles"
    grown_host = psutil.Process().memory_info().rss - rss0
    assert grown_host <= 96 << 20, f"host memory grew by {grown_host / 2**20:.1f} MiB over 50 chain handles"
