"""TEST INFRASTRUCTURE for the Fuse runs on points named as map-store slots (dvm_fuse_targets_run[_hits]_resident,
dvm_fuse_targets_run_hits_candidates): the records of a scene's points, the table the uploaded run takes for a slot list, and the numpy
restatement of vpFuseCandidates (reference src/LocalMapping.cc:826-846) next to the plain loop it restates."""
import numpy as np

from dvm_slam_amd import capi


def records(pts, bad=None):
    """The dvm_local_point records of a scene's points (n_obs = 1; bad as given)."""
    n = len(pts["pos"])
    r = np.zeros(n, capi.LOCAL_POINT_DTYPE)
    for k in ("pos", "normal", "min_dist", "max_dist", "desc"):
        r[k] = pts[k]
    r["n_obs"] = 1
    if bad is not None:
        r["bad"] = bad
    return r


def table(recs, slots, valid=None):
    """What dvm_fuse_targets_run takes for the rows dvm_fuse_targets_run_resident searches: recs = MapStore.read of the slots >= 0 (in
    their order), a row of zeros for a slot of -1, valid = slot >= 0 and not bad and the caller's valid."""
    slots = np.asarray(slots, np.int32)
    n = len(slots)
    named = slots >= 0
    full = np.zeros(n, capi.LOCAL_POINT_DTYPE)
    full[named] = recs
    v = named & (full["bad"] == 0)
    if valid is not None:
        v &= np.asarray(valid).astype(bool)
    return dict(pos=full["pos"].copy(), normal=full["normal"].copy(), min_dist=full["min_dist"].copy(), max_dist=full["max_dist"].copy(),
                desc=full["desc"].copy(), valid=v.astype(np.uint8))


def read_table(store, slots, valid=None):
    slots = np.asarray(slots, np.int32)
    named = slots[slots >= 0]
    recs = store.read(named) if len(named) else np.zeros(0, capi.LOCAL_POINT_DTYPE)
    return table(recs, slots, valid)


def candidates(lists, bad):
    """vpFuseCandidates as slots: the entries numbered flat in (list, keypoint) order; a candidate names a slot >= 0 whose point is not
    bad and that no earlier entry names; flat order kept.  bad [capacity]."""
    flat = np.concatenate([np.asarray(a, np.int32).reshape(-1) for a in lists]) if len(lists) else np.zeros(0, np.int32)
    bad = np.asarray(bad).astype(bool)
    ok = np.flatnonzero(flat >= 0)
    ok = ok[~bad[flat[ok]]]
    _, first = np.unique(flat[ok], return_index=True)
    return flat[ok[np.sort(first)]].astype(np.int32)


def candidates_loop(lists, bad, kf_id=7):
    """LocalMapping.cc:826-846 line for line: a map point is a slot, NULL is -1, mnFuseCandidateForKF a dict."""
    fuse_candidate_for_kf = {}
    vpFuseCandidates = []
    for vpMapPointsKFi in lists:                    # for every target keyframe: GetMapPointMatches()
        for pMP in vpMapPointsKFi:
            pMP = int(pMP)
            if pMP < 0:                             # if (!pMP) continue;
                continue
            if bad[pMP] or fuse_candidate_for_kf.get(pMP) == kf_id:
                continue
            fuse_candidate_for_kf[pMP] = kf_id
            vpFuseCandidates.append(pMP)
    return np.array(vpFuseCandidates, np.int32)
