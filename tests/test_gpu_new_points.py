"""dvm_create_new_map_points (LocalMapping::CreateNewMapPoints for all neighbours as one device chain) against the oracle composition
(tests/new_points_scene.oracle_chain), against the loop of the separate HIP calls it reschedules, and against its own host entry.
Kernel and oracle run one operation sequence, so every field is compared exactly and x3D bit for bit.  The scenes are pinned by
tests/test_oracle_new_points.py (CPU)."""
import functools

import numpy as np
import pytest

import new_points_scene as nps

pytestmark = pytest.mark.gpu

SEEDS = (0, 1)
VARIANTS = {
    "plain": dict(),
    "check_ori": dict(check_ori=True),
    "coarse": dict(coarse=True),
    "coarse_ori": dict(coarse=True, check_ori=True),
    "far": dict(far_points=True, th_far=9.0),
    "inertial": dict(cos_parallax_max=0.9996),
}


@functools.lru_cache(maxsize=None)
def _oracle(seed, n, variant):
    return nps.oracle_chain(nps.prefix(nps.scene(seed), n), **VARIANTS[variant])


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.NewPoints()
    h.reserve(2048, 30, 30 * 1024)
    yield h
    h.close()


def _run(h, sc, **kw):
    return h.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"], **kw)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n", [1, 5, 30])
@pytest.mark.parametrize("seed", SEEDS)
def test_parity_with_oracle(chain, seed, n, variant):
    want = _oracle(seed, n, variant)
    got = _run(chain, nps.prefix(nps.scene(seed), n), **VARIANTS[variant])
    nps.assert_same(got, want)
    if n >= 5:
        assert (got["nb_status"] == 1).sum() >= 1 and (got["status"] == 0).sum() >= 60
    if variant == "far":
        assert (got["status"] == 8).sum() >= 1


def _separate_calls(capi, sc, coarse=False, check_ori=False, cos_parallax_max=0.9998, far_points=False, th_far=0.0):
    """The parent's way: per neighbour capi.search_for_triangulation, then capi.triangulate_matches, the table updated in between."""
    cur, nbs = sc["cur"], sc["neighbours"]
    va = capi.keyframe_view(cur)                                   # (the view reads cur["mp"] in place)
    T1, Ow1 = nps.pose_3x4(cur["Tcw"])
    rf = np.float32(1.5) * np.float32(cur["scale_factors"][1])
    n_nb = len(nbs)
    out = dict(nb_status=np.zeros(n_nb, np.int32), nb_matches=np.zeros(n_nb, np.int32), pair_off=np.zeros(n_nb + 1, np.int32),
               new_point=np.full(len(cur["kps"]), -1, np.int32))
    P, S, Xs = [np.zeros((0, 2), np.int32)], [np.zeros(0, np.int32)], [np.zeros((0, 3), np.float32)]
    base = 0
    for j, nb in enumerate(nbs):
        out["pair_off"][j] = base
        T2, Ow2 = nps.pose_3x4(nb["Tcw"])
        if float(nps.baseline_ratio(Ow1, Ow2, sc["median_depth"][j])) < 0.01:
            out["nb_status"][j] = 1
            continue
        n, pairs = capi.search_for_triangulation(va, capi.keyframe_view(nb), coarse, check_ori)
        out["nb_matches"][j] = n
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        X, st = capi.triangulate_matches(cur["K"], nb["K"], T1, T2, Ow1, Ow2, cur["kps"], nb["kps"], pairs, cur["level_sigma2"], nb["level_sigma2"],
                                         cur["scale_factors"], nb["scale_factors"], rf, cos_parallax_max=cos_parallax_max, far_points=far_points, th_far=th_far)
        ok = np.nonzero(st == 0)[0]
        out["new_point"][pairs[ok, 0]] = base + ok
        cur["mp"][pairs[ok, 0]] = nps.NEW_POINT_ID
        P.append(pairs); S.append(st); Xs.append(X)
        base += len(pairs)
    out["pair_off"][n_nb] = base
    out.update(pairs=np.concatenate(P), status=np.concatenate(S), x3D=np.concatenate(Xs))
    return out


@pytest.mark.parametrize("seed,n,variant", [(0, 30, "plain"), (1, 30, "check_ori"), (0, 5, "coarse_ori"), (1, 5, "far")])
def test_parity_with_the_separate_calls(capi, chain, seed, n, variant):
    """The chain is a rescheduling of the existing HIP calls, not a new result."""
    got = _run(chain, nps.prefix(nps.scene(seed), n), **VARIANTS[variant])
    want = _separate_calls(capi, nps.prefix(nps.scene(seed), n), **VARIANTS[variant])
    nps.assert_same(got, want)
    assert len(got["pairs"]) > 100


@pytest.mark.parametrize("seed,n,variant", [(0, 30, "check_ori"), (1, 5, "plain"), (0, 0, "plain")])
def test_host_entry_equals_device_entry(capi, chain, seed, n, variant):
    sc = nps.prefix(nps.scene(seed), n)
    got = capi.create_new_map_points(sc["cur"], sc["neighbours"], sc["median_depth"], **VARIANTS[variant])
    nps.assert_same(got, _run(chain, sc, **VARIANTS[variant]))
    nps.assert_same(got, _oracle(seed, n, variant))


def _empty_fv(kf):
    kf = dict(kf)
    kf["fv"] = dict(fv_nodes=np.zeros(0, np.int32), fv_off=np.zeros(1, np.int32), fv_feat=np.zeros(0, np.int32))
    return kf


def test_edges(chain):
    sc = nps.prefix(nps.scene(0), 5)
    n1 = len(sc["cur"]["kps"])
    # no neighbours
    r = _run(chain, nps.prefix(nps.scene(0), 0))
    assert r["pairs"].shape == (0, 2) and np.array_equal(r["pair_off"], [0]) and np.all(r["new_point"] == -1) and len(r["new_point"]) == n1
    # every keypoint of the current keyframe mapped: the neighbours run, nobody is asked
    full = nps.prefix(nps.scene(0), 5); full["cur"]["mp"][:] = 7
    r = _run(chain, full)
    assert len(r["pairs"]) == 0 and np.array_equal(r["nb_status"], [0, 1, 0, 0, 0]) and np.all(r["nb_matches"] == 0) and np.all(r["new_point"] == -1)
    nps.assert_same(r, nps.oracle_chain(full))
    # a neighbour with an empty feature vector (and a current keyframe with one)
    e = nps.prefix(nps.scene(0), 5); e["neighbours"] = list(e["neighbours"]); e["neighbours"][2] = _empty_fv(e["neighbours"][2])
    r = _run(chain, e, check_ori=True)
    nps.assert_same(r, nps.oracle_chain(e, check_ori=True))
    assert r["nb_matches"][2] == 0 and r["nb_status"][2] == 0 and r["nb_matches"][0] > 20
    e = nps.prefix(nps.scene(0), 5); e["cur"] = _empty_fv(e["cur"])
    assert len(_run(chain, e)["pairs"]) == 0
    # all neighbours skipped by the baseline test
    s = nps.prefix(nps.scene(0), 5); s["median_depth"][:] = 1e6
    r = _run(chain, s)
    assert np.all(r["nb_status"] == 1) and len(r["pairs"]) == 0 and np.all(r["pair_off"] == 0) and np.all(r["new_point"] == -1)
    # an octave of the current keyframe outside the tables: status -1, a zero point, the keypoint stays free for the next neighbour
    base = _oracle(0, 5, "plain")
    i1 = int(base["pairs"][0, 0])
    o = nps.prefix(nps.scene(0), 5); o["cur"]["kps"] = o["cur"]["kps"].copy(); o["cur"]["kps"]["octave"][i1] = 9
    r = _run(chain, o)
    rows = np.nonzero(r["pairs"][:, 0] == i1)[0]
    assert len(rows) >= 1 and np.all(r["status"][rows] == -1) and np.all(r["x3D"][rows] == 0) and r["new_point"][i1] == -1
    keep = r["pairs"][:, 0] != i1
    assert np.array_equal(r["status"][keep], base["status"][base["pairs"][:, 0] != i1])


def test_refusals_leave_the_handle_usable(capi):
    h = capi.NewPoints()
    h.reserve(1024, 5, 5 * 1024)
    sc = nps.prefix(nps.scene(1), 5)
    want = _oracle(1, 5, "plain")

    def refused(code, scene, **kw):
        with pytest.raises(capi.DvmError) as e:
            _run(h, scene, **kw)
        assert e.value.code == code, str(e.value)
        nps.assert_same(_run(h, sc), want)                        # ... and the next call is served

    refused(-3, nps.prefix(nps.scene(1), 6))                      # more neighbours than reserved
    small = capi.NewPoints(); small.reserve(1024, 5, 500)         # the neighbours' keypoints beyond the reservation
    with pytest.raises(capi.DvmError) as e:
        _run(small, sc)
    assert e.value.code == -3
    small.close()
    refused(-3, sc, record_cap=10)                                # the caller's record arrays too small
    big = nps.prefix(nps.scene(1), 5); big["neighbours"] = list(big["neighbours"])
    kf = big["neighbours"][2]
    n = 8193
    big["neighbours"][2] = dict(kf, kps=np.zeros(n, capi.KP_DTYPE), desc=np.zeros((n, 32), np.uint8), mp=np.full(n, -1, np.int32))
    refused(-1, big)                                              # n > 8192

    def with_fv(j, **changes):
        s = nps.prefix(nps.scene(1), 5); s["neighbours"] = list(s["neighbours"])
        kf = s["cur"] if j < 0 else s["neighbours"][j]
        fv = {k: v.copy() for k, v in kf["fv"].items()}
        for k, (i, v) in changes.items():
            fv[k][i] = v
        kf = dict(kf, fv=fv)
        if j < 0:
            s["cur"] = kf
        else:
            s["neighbours"][j] = kf
        return s
    refused(-1, with_fv(3, fv_off=(4, 0)))                        # offsets not monotone
    refused(-1, with_fv(-1, fv_off=(2, 10 ** 6)))
    refused(-1, with_fv(0, fv_feat=(5, len(sc["neighbours"][0]["kps"]))))   # a feature index out of range
    refused(-1, with_fv(-1, fv_feat=(0, -1)))
    refused(-1, sc, monocular=0)
    h.close()


def test_reuse_no_stale_rows_and_repeatable(capi):
    h = capi.NewPoints()
    h.reserve(2048, 30, 30 * 1024)
    big = _run(h, nps.prefix(nps.scene(0), 30), check_ori=True)
    nps.assert_same(big, _oracle(0, 30, "check_ori"))
    small = _run(h, nps.prefix(nps.scene(1), 5), check_ori=True)   # a smaller problem on the same handle: its solo result
    nps.assert_same(small, _oracle(1, 5, "check_ori"))
    again = _run(h, nps.prefix(nps.scene(1), 5), check_ori=True)
    for k in small:
        assert small[k].tobytes() == again[k].tobytes(), k
    h.close()


def test_handles_release_their_memory(capi):
    import psutil
    import torch

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free
    sc = nps.prefix(nps.scene(0), 5)

    def cycle():
        h = capi.NewPoints()
        h.reserve(1024, 5, 5 * 1024)
        _run(h, sc)
        h.reserve(2048, 30, 30 * 1024)
        _run(h, sc)
        h.close()
    cycle(); cycle()
    base, rss0 = used(), psutil.Process().memory_info().rss
    for _ in range(40):
        cycle()
    grown = used() - base
    assert grown <= 8 << 20, f"{grown / 2**20:.1f} MiB of device memory not returned after 40 chain handles"
    grown_host = psutil.Process().memory_info().rss - rss0
    assert grown_host <= 96 << 20, f"host memory grew by {grown_host / 2**20:.1f} MiB over 40 chain handles"
