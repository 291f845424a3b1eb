"""dvm_track_local_map_batch (TrackerBatch.track_local_map): Tracking::TrackLocalMap of several agents' frames of one camera tick as ONE
device chain behind the batched first half.  Every completed frame's outputs equal Tracker.track + Tracker.track_local_map on that frame
alone, bit for bit; frames the first half did not complete are skipped.  Also the sizing of the batched first half's query block when
max_queries is not a multiple of 64."""
import ctypes as C

import numpy as np
import pytest

import pixel_scene as ps
from test_gpu_track_local_map import BOUNDS, KC, _check, _local_points, _mps, _scene_table, _separate, _tcw7f

pytestmark = pytest.mark.gpu

SENT_MP, SENT_OUT = -7, 0xA5


def _raw_batch(capi, t, ext, tables, fms, ths, fars, thfs, want_tp=True):
    """dvm_track_local_map_batch through ctypes with sentinel-filled outputs: (rc, res, status, mp, outlier, track_pts)."""
    count = len(tables)
    ins = (capi.LocalMapIn * count)(); outs = (capi.LocalMapOut * count)(); res = (capi.TrackLocalResult * count)()
    status = np.full(count, 99, np.int32)
    keep, mp, outl, tp = [], [], [], []
    for b in range(count):
        pts = np.ascontiguousarray(tables[b], capi.LOCAL_POINT_DTYPE); fm = np.ascontiguousarray(fms[b], np.int32)
        mp.append(np.full(len(fm), SENT_MP, np.int32)); outl.append(np.full(len(fm), SENT_OUT, np.uint8))
        tp.append(np.zeros(max(len(pts), 1), capi.TRACK_DTYPE))
        keep.append((pts, fm))
        ins[b].pts, ins[b].n, ins[b].frame_mp = (pts.ctypes.data if len(pts) else None), len(pts), fm.ctypes.data
        ins[b].th, ins[b].far_points, ins[b].th_far = float(ths[b]), int(fars[b]), float(thfs[b])
        outs[b].mp_out, outs[b].outlier = mp[b].ctypes.data, outl[b].ctypes.data
        outs[b].track_pts = tp[b].ctypes.data if want_tp else None
    f = capi.lib().dvm_track_local_map_batch
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = f(t, ext.h, count, ins, outs, res, status.ctypes.data)
    return rc, res, status, mp, outl, [x[:len(k[0])] for x, k in zip(tp, keep)]


def _as_dict(r, mp, outl, tp):
    d = {k: getattr(r, k) for k in ("n_to_match", "nmatches", "n_requeried", "n_cleared_bad", "n_edges", "n_inliers", "matches_inliers")}
    d.update(mp=mp, outlier=outl, track_pts=tp, pose=np.array(r.pose[:], np.float64), Tcw=np.array(r.Tcw[:], np.float32))
    return d


def _equal(a, b):
    _check(a, b, exact=True)
    assert a["n_requeried"] == b["n_requeried"]
    assert np.array_equal(a["Tcw"], b["Tcw"])


def _dense_agent(capi, ext, frames, t, scale, rng):
    """agent on the dense stream at frame t: the local map of frames t-3..t-1, LastFrame = frame t-1 (its points the table's last entries)"""
    tabs = []
    for f in (t - 3, t - 2, t - 1):
        n0, k0, d0, _ = ext.extract(frames[f])
        z = rng.uniform(3, 9, n0)
        X = np.column_stack([(k0["x"] - KC[2]) / KC[0] * z, (k0["y"] - KC[3]) / KC[1] * z, z])
        tabs.append(_local_points(capi, k0, d0, X, np.zeros(3), scale, rng, p_obs0=0.1, p_bad=0.02))
        last = k0.copy()
    pts = np.concatenate(tabs)
    n0 = len(tabs[-1])
    return pts, (last, np.arange(len(pts) - n0, len(pts), dtype=np.int32))


def test_batch_equals_single_frames():
    from dvm_slam_amd import capi, synth
    from oracle import pyoracle as po
    B = 6
    ext1 = capi.OrbExtractor(max_batch=1)
    extB = capi.OrbExtractor(max_batch=B)
    tab = ext1.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    trk1 = capi.Tracker(ext1)
    trkB = capi.TrackerBatch(extB, B)
    dense = synth.frame_stream(12)
    rng = np.random.default_rng(31)
    ths = [1.0, 5.0, 15.0, 1.0, 5.0, 1.0]
    fars = [0, 0, 0, 1, 0, 0]
    imgs, Ts, lasts, tables = [], [], [], []
    for b in range(B):
        frames, t = dense, 3 + b
        pts, (kl, ml) = _dense_agent(capi, ext1, frames, t, scale, rng)
        if b == 1:          # above 10 000 entries: the table and perturbed copies
            big = np.concatenate([pts] * 4)[:10500].copy()
            big["pos"][len(pts):] += rng.normal(0, 0.02, (len(big) - len(pts), 3)).astype(np.float32)
            pts = big
        if b == 4:          # very few map points in LastFrame: fewer than 20 matches even with the doubled window
            ml = ml.copy(); ml[rng.random(len(ml)) < 0.998] = -1
        imgs.append(frames[t]); Ts.append(np.array([0, 0, 0, 1, 0.002 * b, 0, 0], np.float32))
        lasts.append((kl, ml, None, _mps(capi, pts))); tables.append(pts)
    thfs = [float(np.median(np.linalg.norm(tables[3]["pos"], axis=1))) if f else 0.0 for f in fars]
    total = sum((len(t) + 63) // 64 * 64 for t in tables)
    trkB.reserve_local_map(total)
    trk1.reserve_local_map(max(len(t) for t in tables))
    ins, keep = trkB.prepare(Ts, lasts)
    got = trkB.track(np.stack(imgs), ins, KC, BOUNDS, scale, inv_s2, th=15.0)
    assert got[4]["tracked"] == 0 and sum(g["tracked"] for g in got) == B - 1, [g["tracked"] for g in got]
    got = [dict(g, kps_un=g["kps_un"].copy(), desc=g["desc"].copy(), mp=g["mp"].copy()) for g in got]
    fms = [np.full(len(g["mp"]), -1, np.int32) if b == 0 else g["mp"] for b, g in enumerate(got)]
    tables[0] = tables[0][:0]           # agent 0: an empty table (its frame holds nothing)
    rc, res, status, mp, outl, tp = _raw_batch(capi, trkB.t, extB, tables, fms, ths, fars, thfs)
    capi.check(rc)
    assert list(status) == [0, 0, 0, 0, 1, 0], list(status)          # DVM_TRACK_FEW_MATCHES echoed
    assert np.all(mp[4] == SENT_MP) and np.all(outl[4] == SENT_OUT)
    r4 = res[4]
    assert all(getattr(r4, k) == 0 for k in ("n_to_match", "nmatches", "n_edges", "n_inliers", "matches_inliers")) and not any(r4.pose[:])
    requeried = 0
    for b in range(B):
        if b == 4:
            continue
        kl, ml, _, mps = lasts[b]
        one = trk1.track(imgs[b], Ts[b], KC, BOUNDS, scale, inv_s2, kl, ml, None, mps, th=15.0)
        assert one["tracked"] and np.array_equal(one["mp"], got[b]["mp"])
        single = trk1.track_local_map(tables[b], fms[b], th=ths[b], far_points=bool(fars[b]), th_far=thfs[b], want_track_points=True)
        batch = _as_dict(res[b], mp[b], outl[b], tp[b])
        _equal(batch, single)
        requeried += batch["n_requeried"]
        if b == 2:          # and the oracle composition
            orc = _separate(po, got[b]["kps_un"], got[b]["desc"], fms[b], tables[b], got[b]["Tcw"], KC, BOUNDS, scale, inv_s2, ths[b],
                            bool(fars[b]), thfs[b])
            _check(batch, orc, exact=False)
    assert res[0].nmatches == 0 and res[0].n_edges == 0
    assert res[1].n_to_match > 3000 and res[1].nmatches > 0
    assert requeried > 0
    trkB.close(); trk1.close(); extB.close(); ext1.close()


def test_chained_ticks_equal_single_frames():
    """4 agents x 10 ticks: each agent's two halves feed its next LastFrame; the batched loop equals the per-agent single-frame loop."""
    from dvm_slam_amd import capi
    frames, poses = ps.render(12)
    A = 4
    ext1 = capi.OrbExtractor(max_batch=1)
    extB = capi.OrbExtractor(max_batch=A)
    tab = ext1.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    K = ps.K.astype(np.float32)
    tables, state = [], {}
    for a in range(A):
        rng = np.random.default_rng(40 + a)
        pts, (k0, n0) = _scene_table(capi, ext1, frames, poses, scale, rng, ids=(0, 2, 4, 6, 8))
        pts["bad"] = 0
        tables.append(pts)
        for mode in ("batch", "single"):
            state[mode, a] = (k0, np.arange(n0, dtype=np.int32), None, _tcw7f(ps.pose7(*poses[0])))
    trk1 = capi.Tracker(ext1)
    trk1.reserve_local_map(max(len(t) for t in tables))
    trkB = capi.TrackerBatch(extB, A)
    trkB.reserve_local_map(sum((len(t) + 63) // 64 * 64 for t in tables))
    mpss = [_mps(capi, t) for t in tables]
    for t in range(1, 11):
        ins, keep = trkB.prepare([state["batch", a][3] for a in range(A)], [state["batch", a][:3] + (mpss[a],) for a in range(A)])
        first = trkB.track(np.stack([frames[t]] * A), ins, K, BOUNDS, scale, inv_s2, th=15.0)
        assert all(f["tracked"] for f in first)
        sec = trkB.track_local_map(tables, [f["mp"] for f in first], th=1.0)
        for a in range(A):
            r = sec[a]
            assert r["status"] == 0
            state["batch", a] = (first[a]["kps_un"].copy(), r["mp"].copy(), r["outlier"].copy(),
                                 np.concatenate([r["pose"][3:7], r["pose"][0:3]]).astype(np.float32))
            kl, ml, ol, T = state["single", a]
            f1 = trk1.track(frames[t], T, ps.K, BOUNDS, scale, inv_s2, kl, ml, ol, mpss[a], th=15.0)
            r1 = trk1.track_local_map(tables[a], f1["mp"], th=1.0)
            state["single", a] = (f1["kps_un"].copy(), r1["mp"].copy(), r1["outlier"].copy(),
                                  np.concatenate([r1["pose"][3:7], r1["pose"][0:3]]).astype(np.float32))
            x, y = state["batch", a], state["single", a]
            assert np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3]), (t, a)
            assert np.array_equal(r["pose"], r1["pose"])
    gt = ps.pose7(*poses[10])
    for a in range(A):
        assert np.abs(state["batch", a][3][4:7] - gt[:3]).max() < 0.05, a
    trkB.close(); trk1.close(); extB.close(); ext1.close()


def test_requeried_queries_equal_single_calls():
    """Dense stream, th = 15: the device re-scans windows in the batch as the single call does."""
    from dvm_slam_amd import capi, synth
    B = 3
    ext1 = capi.OrbExtractor(max_batch=1)
    extB = capi.OrbExtractor(max_batch=B)
    tab = ext1.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    frames = synth.frame_stream(8)
    rng = np.random.default_rng(9)
    imgs, lasts, tables = [], [], []
    for b in range(B):
        pts, (kl, ml) = _dense_agent(capi, ext1, frames, 3 + b, scale, rng)
        imgs.append(frames[3 + b]); lasts.append((kl, ml, None, _mps(capi, pts))); tables.append(pts)
    Tcw = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    trkB = capi.TrackerBatch(extB, B)
    trkB.reserve_local_map(B * 4096)
    trk1 = capi.Tracker(ext1)
    trk1.reserve_local_map(4096)
    ins, keep = trkB.prepare([Tcw] * B, lasts)
    first = trkB.track(np.stack(imgs), ins, KC, BOUNDS, scale, inv_s2, th=15.0)
    got = trkB.track_local_map(tables, [f["mp"] for f in first], th=15.0)
    total = 0
    for b in range(B):
        assert got[b]["status"] == 0
        kl, ml, _, mps = lasts[b]
        f1 = trk1.track(imgs[b], Tcw, KC, BOUNDS, scale, inv_s2, kl, ml, None, mps, th=15.0)
        one = trk1.track_local_map(tables[b], f1["mp"], th=15.0)
        assert got[b]["n_requeried"] == one["n_requeried"]
        assert np.array_equal(got[b]["mp"], one["mp"]) and np.array_equal(got[b]["pose"], one["pose"])
        total += got[b]["n_requeried"]
    assert total > 0
    trkB.close(); trk1.close(); extB.close(); ext1.close()


@pytest.mark.parametrize("distorted", [False, True])
def test_batch_of_one_equals_single_call(distorted):
    from dvm_slam_amd import capi
    frames, poses = ps.render(4)
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    rng = np.random.default_rng(11)
    pts, (k0, n0) = _scene_table(capi, ext, frames, poses, scale, rng)
    dist, bounds = None, BOUNDS
    if distorted:
        cam = np.array([500.0, 500.0, 320.0, 240.0, -0.04, 0.01, 0.0005, -0.0003, 0.0], np.float32)
        dist = capi.Distortion(*[float(v) for v in cam])
        bounds = capi.image_bounds(cam, 640, 480)
    trk = capi.Tracker(ext)
    trk.reserve_local_map(len(pts))
    mps = _mps(capi, pts)

    def first_half():
        f = trk.track(frames[1], _tcw7f(ps.pose7(*poses[0])), ps.K, bounds, scale, inv_s2, k0, np.arange(n0, dtype=np.int32), None, mps,
                      th=15.0, dist=dist)
        assert f["tracked"]
        return f
    f = first_half()
    single = trk.track_local_map(pts, f["mp"], th=5.0, want_track_points=True)
    f2 = first_half()
    assert np.array_equal(f["mp"], f2["mp"])
    rc, res, status, mp, outl, tp = _raw_batch(capi, trk.t, ext, [pts], [f2["mp"]], [5.0], [0], [0.0])
    capi.check(rc)
    assert status[0] == 0
    _equal(_as_dict(res[0], mp[0], outl[0], tp[0]), single)
    assert single["nmatches"] > 0
    trk.close(); ext.close()


def test_state_and_capacity():
    import torch
    from dvm_slam_amd import capi, synth
    B = 3
    extB = capi.OrbExtractor(max_batch=B)
    ext2 = capi.OrbExtractor(max_batch=B)
    tab = extB.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    frames = synth.frame_stream(7)
    rng = np.random.default_rng(13)
    imgs, lasts, tables = [], [], []
    for b in range(B):
        pts, (kl, ml) = _dense_agent(capi, extB, frames, 3 + b, scale, rng)
        imgs.append(frames[3 + b]); lasts.append((kl, ml, None, _mps(capi, pts))); tables.append(pts)
    Tcw = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    trkB = capi.TrackerBatch(extB, B)
    ins, keep = trkB.prepare([Tcw] * B, lasts)

    def first():
        r = trkB.track(np.stack(imgs), ins, KC, BOUNDS, scale, inv_s2, th=15.0)
        assert all(x["tracked"] for x in r)
        return [x["mp"].copy() for x in r]

    def code(fn):
        with pytest.raises(capi.DvmError) as e:
            fn()
        return e.value.code
    fms = first()
    assert code(lambda: trkB.track_local_map(tables, fms)) == -6                  # no reservation
    trkB.reserve_local_map(B * 4096)
    assert code(lambda: trkB.track_local_map(tables, fms)) == -6                  # no finish since the reservation
    fms = first()
    assert code(lambda: trkB.track_local_map(tables[:2], fms[:2])) == -6          # count differs from the finish's
    assert code(lambda: _check_rc(capi, _raw_batch(capi, trkB.t, ext2, tables, fms, [1] * B, [0] * B, [0] * B))) == -6   # another extractor
    # the single call refuses after a multi-frame finish
    assert code(lambda: capi.Tracker.track_local_map(trkB, tables[0], fms[0])) == -6
    bad = [f.copy() for f in fms]
    bad[1][0] = len(tables[1])
    assert code(lambda: trkB.track_local_map(tables, bad)) == -1                 # frame_mp outside the table
    big = [np.concatenate([t, t])[:4100] for t in tables]                         # 3 x 4 160 > 12 288 reserved
    assert code(lambda: trkB.track_local_map(big, fms)) == -3
    ok = trkB.track_local_map(tables, fms)                                        # the frames are still there for a call that fits
    assert all(r["status"] == 0 and r["nmatches"] > 0 for r in ok)
    assert code(lambda: trkB.track_local_map(tables, fms)) == -6                  # once per finish
    fms = first()
    img = np.ascontiguousarray(np.stack(imgs))
    L = capi.lib()
    L.dvm_track_begin_batch.restype = C.c_int32
    L.dvm_track_begin_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]
    capi.check(L.dvm_track_begin_batch(trkB.t, extB.h, img.ctypes.data, B, 480, 640, img.strides[1], img.strides[0], 0, 1000))
    assert code(lambda: trkB.track_local_map(tables, fms)) == -6                  # after a begin
    extB.sync()
    trkB.close(); ext2.close()
    # a 32-frame tracker takes 32 x 16 384 entries, and reservations release their memory
    ext32 = capi.OrbExtractor(max_batch=32)

    def cycle():
        t = capi.TrackerBatch(ext32, 32)
        t.reserve_local_map(32 * 16384)
        t.reserve_local_map(32 * 4096)            # a second reservation replaces the first
        t.close()

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free
    cycle(); cycle()
    base = used()
    for _ in range(10):
        cycle()
    grown = used() - base
    assert grown <= 8 << 20, f"{grown / 2**20:.1f} MiB of device memory not returned after 10 batched reservations"
    ext32.close(); extB.close()


def _check_rc(capi, r):
    capi.check(r[0])


def test_batched_first_half_beyond_rounded_query_capacity():
    """max_queries not a multiple of 64 and more than round_down(max_queries, 64) queries: the batched first half's query block and ranked
    lists are sized for the call's stride (max_queries rounded up to 64).  Never run against a library without the fix."""
    from dvm_slam_amd import capi, synth
    if not hasattr(capi.lib(), "dvm_track_local_map_batch"):
        pytest.skip("library without the batched second half (and the query block sizing fix)")
    B = 2
    ext1 = capi.OrbExtractor(nfeatures=1100, max_batch=1)
    extB = capi.OrbExtractor(nfeatures=1100, max_batch=B)
    MAXQ, NQ = 1000, 990
    tab = ext1.tables()
    scale, inv_s2 = tab["scale"], tab["inv_sigma2"]
    frames = synth.frame_stream(4)
    rng = np.random.default_rng(3)
    imgs, lasts = [], []
    for b in range(B):
        n0, k0, d0, _ = ext1.extract(frames[b])
        assert n0 > NQ, n0
        z = rng.uniform(3, 9, n0).astype(np.float32)
        mps = np.zeros(n0, capi.MAP_POINT_DTYPE)
        mps["pos"][:, 0] = (k0["x"] - KC[2]) / KC[0] * z; mps["pos"][:, 1] = (k0["y"] - KC[3]) / KC[1] * z; mps["pos"][:, 2] = z
        mps["desc"] = d0; mps["n_obs"] = 1
        ml = np.arange(n0, dtype=np.int32); ml[NQ:] = -1       # NQ queries: more than round_down(MAXQ, 64) = 960
        imgs.append(frames[b + 1]); lasts.append((k0.copy(), ml, None, mps))
    Tcw = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    trk1 = capi.Tracker(ext1)
    trkB = capi.TrackerBatch(extB, B)
    trkB.close()                      # the same tracker with max_queries = 1000 (not a multiple of 64)
    f = capi.lib().dvm_tracker_create_batch
    f.restype = C.c_int32; f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    trkB.t = C.c_void_p()
    capi.check(f(0, B, extB.cap, MAXQ, C.byref(trkB.t)))
    ins, keep = trkB.prepare([Tcw] * B, lasts)
    got = trkB.track(np.stack(imgs), ins, KC, BOUNDS, scale, inv_s2, th=15.0)
    for b in range(B):
        kl, ml, _, mps = lasts[b]
        one = trk1.track(imgs[b], Tcw, KC, BOUNDS, scale, inv_s2, kl, ml, None, mps, th=15.0)
        for k in ("n", "nmatches", "nmatches_search", "nmatches_map", "n_inliers", "tracked", "n_requeried"):
            assert got[b][k] == one[k], (b, k)
        assert np.array_equal(got[b]["mp"], one["mp"]) and np.array_equal(got[b]["dropped"], one["dropped"])
        assert np.array_equal(got[b]["pose"], one["pose"])
    trkB.close(); trk1.close(); extB.close(); ext1.close()
