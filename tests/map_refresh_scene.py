"""TEST INFRASTRUCTURE for dvm_map_store_refresh (a map point's record made on the resident stores): scenes whose observations ARE keypoints
of keyframes in a KeyframeStore and whose points ARE MapStore records, and the float32 numpy restatement of what a refresh leaves --
MapPoint::ComputeDistinctiveDescriptors over the observations on keyframes that are not bad (MapPoint.cc:384-453) and
MapPoint::UpdateNormalAndDepth over all of them (:473-540), one rounding per operation, the sum in list order.  host_path() is the path
an integrator has without the call: gather the rows, dvm_distinctive_descriptors, build the record, MapStore.update.
tests/test_map_refresh_scene.py checks this module on the CPU."""
import numpy as np

from ba_resident_scene import TABLES_A, TABLES_B, norm3, sum3  # noqa: F401  (sum3: the association norm3 is built on)
from dvm_slam_amd import capi
from keyframe_store_scene import keyframe

F32 = np.float32
BAD, DESCRIPTOR, GEOMETRY, BOTH = 1, 1, 2, 3


def make_keyframe(seed, n, tables=TABLES_A):
    """keyframe_store_scene.keyframe with the given level tables (octaves folded into them)."""
    kf = keyframe(seed, n, fv=False)
    kf.update(tables)
    kf["kps"]["octave"] %= len(tables["scale_factors"])
    return kf


def make_scene(seed, kfs, counts, bad=(), gone=(), new=(), ref=None, distinct=True, kf_of=None, kp_of=None):
    """Points with counts[p] observations each on the keyframes kfs (dicts).  bad: keyframe indices flagged DVM_MPR_KF_BAD; gone: those
    of them that carry slot = -1.  new: point indices that enter the store with the call.  ref: per point "first" / "last" / "mid" or an
    index (default: random among the observations on keyframes that still have a slot).  distinct: a point's observations lie on distinct keyframes while
    there are enough of them; kf_of / kp_of: {point: its observations' keyframes / keypoints} instead of drawn ones.  Every keyframe's keypoints 0 and n - 1 are observed by some point when the counts allow it."""
    rng = np.random.default_rng([seed, len(kfs), len(counts), 39])
    K, n = len(kfs), len(counts)
    bad_flag = np.zeros(K, bool); bad_flag[list(bad)] = True
    gone_flag = np.isin(np.arange(K), list(gone))
    obs_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    obs = np.zeros(obs_off[-1], capi.MP_OBS_DTYPE)
    ref_obs = np.zeros(n, np.int32)
    edge = 0
    for p, N in enumerate(counts):
        o = obs[obs_off[p]:obs_off[p + 1]]
        o["kf"] = rng.permutation(K)[:N] if distinct and N <= K else rng.integers(0, K, N)
        for j in range(N):
            nk = len(kfs[o["kf"][j]]["kps"])
            o["kp"][j] = (0, nk - 1)[edge % 2] if edge < 2 * K and j == 0 else rng.integers(0, nk)
            edge += j == 0
        if kf_of and p in kf_of:
            o["kf"] = kf_of[p]
            o["kp"] = [rng.integers(0, len(kfs[k]["kps"])) for k in kf_of[p]]
        if kp_of and p in kp_of:
            o["kp"] = kp_of[p]
        if N == 0:
            continue
        ok = np.flatnonzero(~gone_flag[o["kf"]])        # the ref needs a slot: any keyframe that has not left the store, bad or not
        if len(ok) == 0:
            o["kf"][0] = np.flatnonzero(~gone_flag)[0]; o["kp"][0] = 0
            ok = np.array([0])
        want = None if ref is None else ref[p] if isinstance(ref, (list, tuple)) else ref
        pick = {"first": ok[0], "last": ok[-1], "mid": ok[len(ok) // 2], None: rng.choice(ok)}.get(want, want)
        ref_obs[p] = pick
    rec = np.zeros(n, capi.LOCAL_POINT_DTYPE)
    rec["pos"] = rng.uniform(-6, 6, (n, 3)).astype(F32) + np.array([0, 0, 9], F32)
    nrm = rng.normal(size=(n, 3)); rec["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    rec["min_dist"] = rng.uniform(0.5, 2.0, n); rec["max_dist"] = rng.uniform(20.0, 40.0, n)
    rec["desc"] = rng.integers(0, 256, (n, 32), dtype=np.uint8); rec["n_obs"] = rng.integers(0, 9, n); rec["bad"] = rng.integers(0, 2, n)
    is_new = np.zeros(n, np.uint8); is_new[list(new)] = 1
    return dict(kfs=kfs, ow=rng.uniform(-2, 2, (K, 3)).astype(F32), bad=bad_flag, gone=gone_flag, obs_off=obs_off, obs=obs,
                ref_obs=ref_obs, records=rec, is_new=is_new, new_pos=(rec["pos"] + rng.normal(0, 0.05, (n, 3))).astype(F32))


def kf_table(sc, kf_slots):
    """the call's dvm_mp_refresh_kf array for keyframes placed at kf_slots"""
    t = np.zeros(len(sc["kfs"]), capi.MP_REFRESH_KF_DTYPE)
    t["slot"] = np.where(sc["gone"], -1, kf_slots); t["flags"] = sc["bad"].astype(np.uint32) * BAD; t["ow"] = sc["ow"]
    return t


def rows_of(sc, p, candidates_only=True):
    """(rows [N', 32], index in the full list [N']) of point p's observations, those on keyframes that are not bad"""
    o = sc["obs"][sc["obs_off"][p]:sc["obs_off"][p + 1]]
    idx = np.flatnonzero(~sc["bad"][o["kf"]]) if candidates_only else np.arange(len(o))
    rows = np.array([sc["kfs"][o["kf"][j]]["desc"][o["kp"][j]] for j in idx], np.uint8).reshape(-1, 32)
    return rows, idx


def hamming_table(rows):
    b = np.unpackbits(np.ascontiguousarray(rows, np.uint8), axis=1).astype(np.int32)
    return b @ (1 - b).T + (1 - b) @ b.T


def distinctive(rows):
    """(winner, median): median_i = sorted_row_i[(N - 1) >> 1], self distance included; the first strictly smaller median wins"""
    N = len(rows)
    if N == 0:
        return -1, -1
    med = np.sort(hamming_table(rows), axis=1)[:, (N - 1) >> 1]
    w = int(np.argmin(med))                             # (the first of equal minima)
    return w, int(med[w])


def geometry(pos, centres, ow_ref, sf_ref, octave_ref):
    """[8] float32: pos, the mean of the unit vectors summed in list order from 0, min_dist, max_dist"""
    pos = np.asarray(pos, F32)
    normal = np.zeros(3, F32)
    for ow in np.asarray(centres, F32).reshape(-1, 3):
        d = (pos - ow).astype(F32)
        normal = (normal + (d / norm3(d)).astype(F32)).astype(F32)
    g = np.zeros(8, F32)
    g[:3] = pos; g[3:6] = normal / F32(len(centres))
    d = (pos - np.asarray(ow_ref, F32)).astype(F32)
    g[7] = F32(norm3(d) * sf_ref[octave_ref])
    g[6] = g[7] / sf_ref[len(sf_ref) - 1]
    return g


def refresh_ref(sc, what=BOTH, winners=None, before=None):
    """What a refresh of every point of the scene leaves: (records [n], best_obs [n], best_median [n], geometry [n, 8]).  winners:
    (index among the candidates, median) per point from elsewhere (dvm_distinctive_descriptors), else the restatement's own.  before: the
    records the slots hold (default the scene's)."""
    n = len(sc["records"])
    rec = (sc["records"] if before is None else before).copy()
    best = np.full(n, -1, np.int32); med = np.full(n, -1, np.int32); geo = np.zeros((n, 8), F32)
    for p in range(n):
        o = sc["obs"][sc["obs_off"][p]:sc["obs_off"][p + 1]]
        N, new = len(o), bool(sc["is_new"][p])
        if new:
            rec[p] = np.zeros((), capi.LOCAL_POINT_DTYPE); rec["pos"][p] = sc["new_pos"][p]
        rec["n_obs"][p] = N
        if (what & DESCRIPTOR) and N:
            rows, idx = rows_of(sc, p)
            w, m = distinctive(rows) if winners is None else winners[p]
            if w >= 0:
                best[p], med[p] = idx[w], m
                rec["desc"][p] = rows[w]
        if (what & GEOMETRY) and N:
            r = o[sc["ref_obs"][p]]
            kf = sc["kfs"][r["kf"]]
            g = geometry(rec["pos"][p], sc["ow"][o["kf"]], sc["ow"][r["kf"]], kf["scale_factors"], kf["kps"]["octave"][r["kp"]])
            rec["normal"][p] = g[3:6]; rec["min_dist"][p] = g[6]; rec["max_dist"][p] = g[7]
        geo[p, :3] = rec["pos"][p]; geo[p, 3:6] = rec["normal"][p]; geo[p, 6] = rec["min_dist"][p]; geo[p, 7] = rec["max_dist"][p]
    return rec, best, med, geo


def host_gather(sc):
    """the upload of today's path: every candidate row of every point, back to back, and its CSR"""
    rows = [rows_of(sc, p)[0] for p in range(len(sc["records"]))]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return (np.concatenate(rows) if off[-1] else np.zeros((0, 32), np.uint8)), off


def host_path(sc, store, mp_slots, what=BOTH, before=None):
    """Today's path on `store`: gather -> capi.distinctive_descriptors -> the restatement's record -> MapStore.update.  Returns what
    refresh_ref returns (the caller reads the store)."""
    desc, off = host_gather(sc)
    bi, bm = capi.distinctive_descriptors(desc, off)
    rec, best, med, geo = refresh_ref(sc, what, winners=list(zip(bi.tolist(), bm.tolist())), before=before)
    store.update(mp_slots, rec)
    return rec, best, med, geo


def call_args(sc, mp_slots, kf_slots):
    """the positional arguments of MapStore.refresh after the keyframe store, and the is_new / new_pos keywords"""
    new = sc["is_new"].any()
    return (mp_slots, sc["obs_off"], sc["obs"], sc["ref_obs"], kf_table(sc, kf_slots)), dict(is_new=sc["is_new"] if new else None, new_pos=sc["new_pos"] if new else None)
