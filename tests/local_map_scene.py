"""Tracking::UpdateLocalMap's two graph walks (reference src/Tracking.cc:3117-3181) restated on a small object graph -- points with an
ordered observation dict and a bad flag, keyframes with a match list --, the rows a dvm_keyframe_store keeps derived from that graph, the
table definitions of include/dvmslam_hip.h (dvm_update_local_map_keyframes / _points) in numpy, and a seeded generator of graphs.

The loops are the checker: they follow the reference statement by statement (the walk over GetObservations() per frame point, the reverse
walk over mvpLocalKeyFrames with the mnTrackReferenceForFrame mark).  The numpy forms are what the device computes, written from the
header's definitions; tests/test_local_map_scene.py holds the two against each other, the GPU tests hold the device against the loops."""
import numpy as np


class MapPoint:
    def __init__(self, slot):
        self.slot = slot
        self.bad = False
        self.observations = {}          # KeyFrame -> keypoint index, in insertion order (GetObservations())
        self.track_reference_for_frame = -1

    def is_bad(self):
        return self.bad

    def add_observation(self, kf, kp):  # MapPoint::AddObservation: one observation per keyframe
        if kf not in self.observations:
            self.observations[kf] = kp


class KeyFrame:
    def __init__(self, slot, n):
        self.slot = slot
        self.matches = [None] * n       # GetMapPointMatches()
        self.bad = False


class Graph:
    """kfs: the keyframes (their slots need not be dense), points: the map points (slot = index into the map store), frame: the current
    frame's mvpMapPoints (MapPoint or None per keypoint), map_capacity / kf_capacity / slot_keypoints: the stores' sizes."""

    def __init__(self, kfs, points, frame, map_capacity, kf_capacity, slot_keypoints):
        self.kfs, self.points, self.frame = kfs, points, frame
        self.map_capacity, self.kf_capacity, self.slot_keypoints = map_capacity, kf_capacity, slot_keypoints

    def frame_slots(self):
        return np.array([-1 if p is None else p.slot for p in self.frame], np.int32)

    def bad_table(self):
        bad = np.zeros(self.map_capacity, bool)
        for p in self.points:
            bad[p.slot] = p.bad
        return bad


# ---- the reference's loops
def update_local_keyframes_votes(frame_points):
    """Tracking.cc:3145-3160 (the branch of :3163-3180 is the same loop on mLastFrame).  frame_points: list of MapPoint / None, cleared in
    place where the point is bad.  Returns keyframeCounter: dict KeyFrame -> votes."""
    keyframe_counter = {}
    for i in range(len(frame_points)):
        p = frame_points[i]
        if p is not None:
            if not p.is_bad():
                observations = dict(p.observations)
                for kf in observations:
                    keyframe_counter[kf] = keyframe_counter.get(kf, 0) + 1
            else:
                frame_points[i] = None
    return keyframe_counter


def update_local_points(local_keyframes, frame_id):
    """Tracking.cc:3117-3141.  local_keyframes: mvpLocalKeyFrames (the loop walks it in reverse).  Returns mvpLocalMapPoints."""
    local_map_points = []
    for kf in reversed(local_keyframes):
        for p in list(kf.matches):
            if p is None:
                continue
            if p.track_reference_for_frame == frame_id:
                continue
            if not p.is_bad():
                local_map_points.append(p)
                p.track_reference_for_frame = frame_id
    return local_map_points


def reference_keyframes(g):
    """What dvm_update_local_map_keyframes must return on graph g: (votes [kf_capacity], frame_bad [n]).  The graph's frame is not modified."""
    frame = list(g.frame)
    counter = update_local_keyframes_votes(frame)
    votes = np.zeros(g.kf_capacity, np.int32)
    for kf, c in counter.items():
        votes[kf.slot] = c
    frame_bad = np.array([a is not None and b is None for a, b in zip(g.frame, frame)], np.uint8).reshape(-1)
    return votes, frame_bad


_frame_ids = iter(range(1, 1 << 30))


def reference_points(g, local_keyframes_visit_order):
    """What dvm_update_local_map_points must return: local_keyframes_visit_order is the order the loop VISITS the keyframes (kf_slot of
    the call; mvpLocalKeyFrames reversed).  Returns (local_slot, frame_mp, n_outside)."""
    local = update_local_points(list(reversed(local_keyframes_visit_order)), next(_frame_ids))
    local_slot = np.array([p.slot for p in local], np.int32)
    where = {p: i for i, p in enumerate(local)}
    frame_mp = np.full(len(g.frame), -1, np.int32)
    n_outside = 0
    for i, p in enumerate(g.frame):
        if p is None or p.is_bad():
            continue
        if p in where:
            frame_mp[i] = where[p]
        else:
            n_outside += 1
    return local_slot, frame_mp, n_outside


# ---- the rows
def row_matches(kf):
    """DVM_KFS_ROW_MATCHES of a keyframe."""
    return np.array([-1 if p is None else p.slot for p in kf.matches], np.int32)


def row_observed(kf, points):
    """DVM_KFS_ROW_OBSERVED: entry kp = the slot of the point whose observations hold (kf, kp)."""
    row = np.full(len(kf.matches), -1, np.int32)
    for p in points:
        kp = p.observations.get(kf)
        if kp is not None:
            row[kp] = p.slot
    return row


# ---- the table definitions in numpy
def votes_table(frame_slots, bad, observed_rows, kf_capacity):
    """observed_rows: dict slot -> OBSERVED row.  mult[s] = the frame's keypoints that hold the non-bad point s; votes[j] = the sum of
    mult over the row's entries.  Returns (votes, frame_bad)."""
    frame_slots = np.asarray(frame_slots, np.int32)
    held = frame_slots >= 0
    frame_bad = np.zeros(len(frame_slots), np.uint8)
    frame_bad[held] = bad[frame_slots[held]]
    mult = np.bincount(frame_slots[held & (frame_bad == 0)], minlength=len(bad)).astype(np.int64)
    votes = np.zeros(kf_capacity, np.int32)
    for j, row in observed_rows.items():
        votes[j] = mult[row[row >= 0]].sum()
    return votes, frame_bad


def local_points_table(kf_slots, matches_rows, bad, frame_slots):
    """The entries are the named slots' MATCHES rows flat in (keyframe, keypoint) order; an entry is taken iff its value is >= 0, its
    record is not bad and no earlier entry names the same slot.  Returns (local_slot, frame_mp, n_outside)."""
    flat = np.concatenate([matches_rows[j] for j in kf_slots] + [np.zeros(0, np.int32)]).astype(np.int32)
    ok = flat >= 0
    ok[ok] = ~bad[flat[ok]]
    cand = flat[ok]
    _, first = np.unique(cand, return_index=True)
    local_slot = cand[np.sort(first)]
    pos = np.full(len(bad), -1, np.int32)
    pos[local_slot] = np.arange(len(local_slot), dtype=np.int32)
    frame_slots = np.asarray(frame_slots, np.int32)
    frame_mp = np.full(len(frame_slots), -1, np.int32)
    live = frame_slots >= 0
    live[live] = ~bad[frame_slots[live]]
    frame_mp[live] = pos[frame_slots[live]]
    return local_slot, frame_mp, int((frame_mp[live] < 0).sum())


# ---- a seeded generator
def make_graph(seed, kf_slots, row_lens, n_points, frame_n, map_capacity, kf_capacity, slot_keypoints, fill=0.6, bad_frac=0.1, queued=(),
               frame_dup=0.1, frame_none=0.15, frame_outside=0.05):
    """Keyframes in slots kf_slots with row_lens keypoints; n_points points in random distinct slots of the map.  A keypoint holds a
    point with probability `fill`; the point observes the keyframe there unless it already observes it elsewhere (a repeat inside the row)
    or the keyframe is in `queued` (indices into kf_slots: matches set, no observation yet).  bad_frac of the points are bad.  The frame
    holds frame_n entries: none, a point of the rows, a repeat of an earlier entry, or a point in no row."""
    rng = np.random.default_rng(seed)
    slots = rng.permutation(map_capacity)[:n_points]
    points = [MapPoint(int(s)) for s in slots]
    n_in_rows = max(1, int(n_points * (1.0 - frame_outside))) if n_points else 0
    in_rows, outside = points[:n_in_rows], points[n_in_rows:]
    kfs = [KeyFrame(int(s), int(n)) for s, n in zip(kf_slots, row_lens)]
    for t, kf in enumerate(kfs):
        for kp in range(len(kf.matches)):
            if not in_rows or rng.random() >= fill:
                continue
            p = in_rows[int(rng.integers(len(in_rows)))]
            kf.matches[kp] = p
            if t not in queued:
                p.add_observation(kf, kp)
    for p in points:
        p.bad = bool(rng.random() < bad_frac)
    frame = []
    for i in range(frame_n):
        u = rng.random()
        if u < frame_none or not points:
            frame.append(None)
        elif u < frame_none + frame_dup and any(f is not None for f in frame):
            held = [f for f in frame if f is not None]
            frame.append(held[int(rng.integers(len(held)))])
        elif u < frame_none + frame_dup + frame_outside and outside:
            frame.append(outside[int(rng.integers(len(outside)))])
        else:
            frame.append(in_rows[int(rng.integers(len(in_rows)))])
    return Graph(kfs, points, frame, map_capacity, kf_capacity, slot_keypoints)


class Placed:
    """Graph g on the device: its keyframes put into a KeyframeStore (tests/keyframe_store_scene keyframes of the rows' lengths), its
    points' records in a MapStore, both rows of every keyframe set (rows=False: none)."""

    def __init__(self, capi, g, rows=True, all_slots=False, device=0):
        import keyframe_store_scene as kss
        self.capi, self.g = capi, g
        self.kfs = capi.KeyframeStore(g.kf_capacity, g.slot_keypoints, device=device)
        self.points = capi.MapStore(g.map_capacity, device=device)
        if g.kfs:
            self.kfs.put([kf.slot for kf in g.kfs], [kss.keyframe(1000 + kf.slot, len(kf.matches)) for kf in g.kfs])
        slots, rec = map_records(g, capi.LOCAL_POINT_DTYPE, all_slots)
        if len(slots):
            self.points.update(slots, rec)
        if rows and g.kfs:
            self.set_rows()

    def set_rows(self, kfs=None):
        kfs = self.g.kfs if kfs is None else kfs
        sl = [kf.slot for kf in kfs]
        self.kfs.set_rows(self.capi.KFS_ROW_MATCHES, self.points, sl, [row_matches(kf) for kf in kfs])
        self.kfs.set_rows(self.capi.KFS_ROW_OBSERVED, self.points, sl, [row_observed(kf, self.g.points) for kf in kfs])

    def frame_keyframes(self, mp_slot=None):
        return dict(kfs=self.kfs, points=self.points, mp_slot=self.g.frame_slots() if mp_slot is None else mp_slot)

    def frame_points(self, order, mp_slot=None):
        return dict(self.frame_keyframes(mp_slot), kf_slot=np.array([kf.slot for kf in order], np.int32))

    def close(self):
        self.kfs.close(); self.points.close()


def map_records(g, dtype, all_slots=False):
    """(slots, records of `dtype` == dvm_local_point) of the graph's points for dvm_map_store_update; all_slots: every slot of the map is
    written (the points' bad flags, the rest not bad)."""
    if all_slots:
        slots = np.arange(g.map_capacity, dtype=np.int32)
    else:
        slots = np.array(sorted(p.slot for p in g.points), np.int32)
    rec = np.zeros(len(slots), dtype)
    bad = g.bad_table()
    rec["bad"] = bad[slots]
    rec["pos"][:, 2] = 1.0
    return slots, rec
