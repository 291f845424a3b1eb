"""TEST INFRASTRUCTURE for dvm_ba_resident (LocalBundleAdjustment windows on the keyframe store and the map store): small windows whose
observations ARE keypoints of keyframes and whose points ARE map-store records, the host-side gather that builds the equivalent
dvm_ba_window (the casts of Optimizer.cc:1188, 1207-1217), and the float32 numpy restatement of the prepare step -- camera centres as
SetPose leaves them (the sequences of csrc/pose_f32.h restated here), dirty flags (Optimizer.cc:1324), SetWorldPos +
MapPoint::UpdateNormalAndDepth (MapPoint.cc:473-540).  tests/test_ba_resident_scene.py checks this module on the CPU."""
import numpy as np

from dvm_slam_amd import capi

F32 = np.float32
HUBER = float(np.sqrt(5.991))
CHI2_ERASE = 5.991
PINHOLE_K = (500.0, 510.0, 320.0, 240.0)
BOUNDS = np.array([0.0, 640.0, 0.0, 480.0], F32)


def level_tables(scale_factor=1.2, n_levels=8):
    s = (F32(scale_factor) ** np.arange(n_levels)).astype(F32)
    return dict(scale_factors=s, level_sigma2=(s * s).astype(F32), inv_level_sigma2=(F32(1.0) / (s * s)).astype(F32),
                log_scale_factor=float(np.log(F32(scale_factor))))


TABLES_A, TABLES_B = level_tables(1.2, 8), level_tables(1.1, 5)


def pinhole():
    return capi.CameraModel.pinhole(*PINHOLE_K)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def _quat(R):
    w = np.sqrt(max(1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1e-12)) / 2     # (small rotations only: w is far from 0)
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def _R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def make_window(seed, P, L, E, n_fixed, model=None, tables=None, unused=0, twice=False, fixed_only=0, outliers=0.0, iterations=5, extra=None,
                behind=0, n_obs=None, noise=0.7):
    """One window.  P cameras a few units apart looking down +z at a cloud 5 to 14 units away, the first n_fixed fixed and exact, the others
    0.003 rad / 0.02 off; L points of which the last `unused` have no edge and the first `fixed_only` are seen by fixed cameras only; exactly E
    edges in random order, every used point at least once while E allows it; twice: the last edge repeats the first edge's (camera, point)
    at another keypoint; outliers: that share of the edges' keypoints is moved by 30 px; behind: that many used points start BEHIND camera 0
    and have one edge only (they stay there: no positive depth); n_obs [L]: the points' observer counts instead (E = their sum; 0: unused);
    noise: px.  tables: per camera (default TABLES_A, every third camera TABLES_B).
    Every observation is a keypoint of its camera's keyframe: x, y = float32(projection + 0.7 px of noise), a random octave -- the first
    edge of camera 0 at octave 0, its last at n_levels - 1 --, at a random index among `extra[p]` (default 5 (p % 3)) other keypoints, so
    camera 0's keypoints are all used: kp = 0 and kp = n - 1 occur."""
    rng = np.random.default_rng([seed, P, L, E, 38])
    model = model or pinhole()
    tables = tables or [TABLES_B if p % 3 == 2 else TABLES_A for p in range(P)]
    gt = np.zeros((P, 7))
    for p in range(P):
        Rm = _rot(rng.normal(size=3), rng.uniform(-0.15, 0.15))
        gt[p] = np.r_[-Rm @ rng.uniform(-1.5, 1.5, 3), _quat(Rm)]
    th = np.deg2rad(25.0) * np.sqrt(rng.uniform(0.0, 1.0, L)); psi = rng.uniform(-np.pi, np.pi, L); d = rng.uniform(5.0, 14.0, L)
    X = np.column_stack([d * np.sin(th) * np.cos(psi), d * np.sin(th) * np.sin(psi), d * np.cos(th)])
    used = L - unused
    for l in range(behind):
        X[used - 1 - l, 2] = -6.0 - l
    pairs, seen = [], set()

    def add(p, l):
        pairs.append((p, l)); seen.add((p, l))
    cams_of = lambda l: range(n_fixed) if l < fixed_only else range(P)     # noqa: E731
    for l in range(L if n_obs is not None else 0):
        for p in rng.permutation(list(cams_of(l)))[:n_obs[l]]:
            add(int(p), l)
    for l in range(0 if n_obs is not None else min(used, E - (1 if twice else 0))):
        add(int(rng.choice(list(cams_of(l)))), l)
    cand = [(p, l) for l in range(0 if n_obs is not None else used - behind) for p in cams_of(l) if (p, l) not in seen]
    rng.shuffle(cand)
    for p, l in cand[:max(E - (1 if twice else 0) - len(pairs), 0)]:
        add(p, l)
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    if twice:
        pairs.append(pairs[0])
    assert len(pairs) == E, (len(pairs), E)
    obs = np.zeros(E, capi.BA_OBS_DTYPE)
    obs["pose"] = [p for p, _ in pairs]; obs["point"] = [l for _, l in pairs]
    uv = np.zeros((E, 2))
    for e, (p, l) in enumerate(pairs):
        Xc = _R(gt[p, 3:]) @ X[l] + gt[p, :3]
        uv[e] = rng.uniform([0.0, 0.0], [640.0, 480.0]) if Xc[2] < 0.1 else model.project(Xc)[0] + rng.normal(0.0, noise, 2)     # (behind: any keypoint)
    out = rng.random(E) < outliers
    uv[out] += rng.choice([-30.0, 30.0], size=(int(out.sum()), 2))
    kfs = []
    for p in range(P):
        mine = np.flatnonzero(obs["pose"] == p)
        n = max(len(mine) + (5 * (p % 3) if extra is None else extra[p]), 1)
        at = rng.permutation(n)[:len(mine)]
        kps = np.zeros(n, capi.KP_DTYPE)
        kps["x"] = rng.uniform(0, 640, n); kps["y"] = rng.uniform(0, 480, n)
        nl = len(tables[p]["scale_factors"])
        kps["octave"] = rng.integers(0, nl, n); kps["angle"] = rng.uniform(0, 360, n); kps["size"] = 31.0; kps["class_id"] = -1
        kps["x"][at] = uv[mine, 0]; kps["y"][at] = uv[mine, 1]
        if p == 0 and len(mine) >= 2:
            kps["octave"][at[0]] = 0; kps["octave"][at[-1]] = nl - 1
        obs["kp"][mine] = at
        kfs.append(dict(kps=kps, desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), K=np.asarray(list(model.p)[:4], F32), bounds=BOUNDS, **tables[p]))
    fixed = np.zeros(P, np.uint8); fixed[:n_fixed] = 1
    poses = gt.copy()
    for p in range(n_fixed, P):
        Rm = _rot(rng.normal(size=3), rng.normal(0.0, 0.003)) @ _R(gt[p, 3:])
        poses[p] = np.r_[gt[p, :3] + rng.normal(0.0, 0.02, 3), _quat(Rm)]
    rec = np.zeros(L, capi.LOCAL_POINT_DTYPE)
    rec["pos"] = (X + rng.normal(0.0, 0.03, (L, 3))).astype(F32)
    nrm = rng.normal(size=(L, 3)); rec["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    rec["min_dist"] = rng.uniform(0.5, 2.0, L); rec["max_dist"] = rng.uniform(20.0, 40.0, L)
    rec["desc"] = rng.integers(0, 256, (L, 32), dtype=np.uint8); rec["n_obs"] = np.bincount(obs["point"], minlength=L); rec["bad"] = 0
    ref = np.full(L, -1, np.int32)
    for l in range(L):
        mine = np.flatnonzero(obs["point"] == l)
        if len(mine):
            ref[l] = rng.choice(mine)
    return dict(P=P, L=L, E=E, poses=poses, fixed=fixed, obs=obs, kfs=kfs, records=rec, ref_edge=ref, model=model, iterations=iterations)


def host_window(sc, use_model=True):
    """The dvm_ba_window the caller of the uploaded form builds from the same keyframes and records: obs << kpUn.pt.x, kpUn.pt.y,
    invSigma2 = mvInvLevelSigma2[kpUn.octave], Vector3d of the float position."""
    o = sc["obs"]
    e = np.zeros(len(o), capi.BA_EDGE_DTYPE)
    e["pose"], e["point"] = o["pose"], o["point"]
    for k in range(len(o)):
        kf = sc["kfs"][o["pose"][k]]
        kp = kf["kps"][o["kp"][k]]
        e["u"][k], e["v"][k] = np.float64(kp["x"]), np.float64(kp["y"])
        e["inv_sigma2"][k] = np.float64(kf["inv_level_sigma2"][kp["octave"]])
    w = dict(poses=sc["poses"], fixed=sc["fixed"], points=sc["records"]["pos"].astype(np.float64), edges=e, huber_delta=HUBER, iterations=sc["iterations"])
    if use_model:
        w["model"] = sc["model"]
    else:
        w["intrinsics"] = [float(v) for v in list(sc["model"].p)[:4]]
    return w


def descending_slots(n, capacity, top=None):
    """n slots descending from `top` (default capacity - 1) with gaps of 1, 2, 1, 2 ..."""
    s = (capacity - 1 if top is None else top) - np.cumsum(np.r_[0, 1 + (np.arange(max(n - 1, 0)) % 2 + 1)])[:n]
    assert n == 0 or s.min() >= 0
    return s.astype(np.int32)


class Placed:
    """The scenes' keyframes and records in a KeyframeStore and a MapStore (new ones, or given ones behind what they hold): slots descending
    with gaps.  problems(): the dicts capi.BaResident.optimize takes."""

    def __init__(self, scenes, kf_store=None, map_store=None, kf_top=None, mp_top=None, ow=None, use_model=True, with_ref=True):
        self.scenes = scenes
        nk = sum(s["P"] for s in scenes); nm = sum(s["L"] for s in scenes)
        slot_kp = max(len(kf["kps"]) for s in scenes for kf in s["kfs"])
        self.kf_store = kf_store or capi.KeyframeStore(3 * nk + 4, max(slot_kp, 64))
        self.map_store = map_store or capi.MapStore(3 * nm + 4)
        ks = descending_slots(nk, self.kf_store.capacity, kf_top); ms = descending_slots(nm, self.map_store.capacity, mp_top)
        self.kf_slots, self.mp_slots, a, b = [], [], 0, 0
        for s in scenes:
            self.kf_slots.append(ks[a:a + s["P"]]); self.mp_slots.append(ms[b:b + s["L"]]); a += s["P"]; b += s["L"]
        self.ow, self.use_model, self.with_ref = ow, use_model, with_ref
        self.upload()

    def upload(self):
        """update -> put, nothing behind them: the optimize that follows must see both"""
        if sum(s["L"] for s in self.scenes):
            self.map_store.update(np.concatenate(self.mp_slots), np.concatenate([s["records"] for s in self.scenes]))
        self.kf_store.put(np.concatenate(self.kf_slots), [kf for s in self.scenes for kf in s["kfs"]])

    def problems(self):
        out = []
        for k, s in enumerate(self.scenes):
            pr = dict(poses=s["poses"], fixed=s["fixed"], kf_slots=self.kf_slots[k], keyframe_store=self.kf_store, mp_slots=self.mp_slots[k], map_store=self.map_store,
                      obs=s["obs"], ref_edge=s["ref_edge"] if self.with_ref else None, ow=None if self.ow is None else self.ow[k], chi2_erase=CHI2_ERASE,
                      huber_delta=HUBER, iterations=s["iterations"])
            if self.use_model:
                pr["model"] = s["model"]
            else:
                pr["intrinsics"] = [float(v) for v in list(s["model"].p)[:4]]
            out.append(pr)
        return out


# ---- csrc/pose_f32.h restated: float32 arrays, one rounding per operation, the header's association
def sum3(a, b, c):
    return a + (b + c)


def sqnorm4(q):
    return (q[..., 0] * q[..., 0] + q[..., 2] * q[..., 2]) + (q[..., 1] * q[..., 1] + q[..., 3] * q[..., 3])


def quat_div(q, d):
    return (q / d[..., None]).astype(F32)


def quat_rotate(q, p):
    a0 = q[..., 1] * p[..., 2] - q[..., 2] * p[..., 1]; a1 = q[..., 2] * p[..., 0] - q[..., 0] * p[..., 2]; a2 = q[..., 0] * p[..., 1] - q[..., 1] * p[..., 0]
    a0 = a0 + a0; a1 = a1 + a1; a2 = a2 + a2
    b0 = q[..., 1] * a2 - q[..., 2] * a1; b1 = q[..., 2] * a0 - q[..., 0] * a2; b2 = q[..., 0] * a1 - q[..., 1] * a0
    return np.stack([(p[..., 0] + q[..., 3] * a0) + b0, (p[..., 1] + q[..., 3] * a1) + b1, (p[..., 2] + q[..., 3] * a2) + b2], axis=-1).astype(F32)


def se3_inverse_t(q, t):
    """the translation of SE3f(q, t).inverse(): the normalised conjugate applied to t * -1"""
    c = np.stack([-q[..., 0], -q[..., 1], -q[..., 2], q[..., 3]], axis=-1).astype(F32)
    qi = quat_div(c, np.sqrt(sqnorm4(c)))
    return quat_rotate(qi, (t * F32(-1.0)).astype(F32))


def camera_centres(poses_in, poses_out, fixed, ow=None):
    """mOw per camera, float32 [P, 3].  Free: the optimised pose cast to float, the quaternion divided by its norm (the SE3f(Quaternionf,
    Vector3f) constructor of Optimizer.cc:1374), inverse().translation().  Fixed: the caller's row, else the same of the input pose as it is."""
    fixed = np.asarray(fixed).astype(bool)
    qo = np.asarray(poses_out)[:, 3:].astype(F32); to = np.asarray(poses_out)[:, :3].astype(F32)
    qo = quat_div(qo, np.sqrt(sqnorm4(qo)))
    free = se3_inverse_t(qo, to)
    held = se3_inverse_t(np.asarray(poses_in)[:, 3:].astype(F32), np.asarray(poses_in)[:, :3].astype(F32))
    if ow is not None:
        held = np.asarray(ow, F32).reshape(-1, 3)
    return np.where(fixed[:, None], held, free).astype(F32)


def norm3(d):
    return np.sqrt(sum3(d[..., 0] * d[..., 0], d[..., 1] * d[..., 1], d[..., 2] * d[..., 2]))


def prepare_ref(sc, res, ow=None, chi2_erase=CHI2_ERASE, with_ref=True, obs=None, ref_edge=None):
    """(geometry [L, 8], point_dirty [L], ow [P, 3], state [L]) from the call's own poses / points / edge_chi2 / depth_positive.
    state: 0 clean and used, 1 dirty, 2 unused; geometry rows of dirty and unused points are zeros."""
    obs = sc["obs"] if obs is None else obs
    ref_edge = sc["ref_edge"] if ref_edge is None else ref_edge
    L = sc["L"]
    centres = camera_centres(sc["poses"], res["poses"], sc["fixed"], ow)
    rejected = (res["edge_chi2"] > np.float64(chi2_erase)) | (res["depth_positive"] == 0)
    geom = np.zeros((L, 8), F32); state = np.zeros(L, np.uint8)
    for l in range(L):
        mine = np.flatnonzero(obs["point"] == l)              # ascending: the caller's order
        if len(mine) == 0:
            state[l] = 2
            continue
        if rejected[mine].any():
            state[l] = 1
            continue
        pos = res["points"][l].astype(F32)
        normal = np.zeros(3, F32)
        for e in mine:
            d = (pos - centres[obs["pose"][e]]).astype(F32)
            normal = (normal + d / norm3(d)).astype(F32)
        geom[l, :3] = pos
        geom[l, 3:6] = normal / F32(len(mine))
        if with_ref:
            r = obs[ref_edge[l]]
            kf = sc["kfs"][r["pose"]]
            d = (pos - centres[r["pose"]]).astype(F32)
            max_dist = F32(norm3(d) * kf["scale_factors"][kf["kps"]["octave"][r["kp"]]])
            geom[l, 7] = max_dist
            geom[l, 6] = max_dist / kf["scale_factors"][len(kf["scale_factors"]) - 1]
    return geom, (state == 1).astype(np.uint8), centres, state


def committed_records(before, geom, state):
    """the records a commit leaves: the geometry words of clean, used points replaced, every other bit as before"""
    out = before.copy()
    ok = state == 0
    out["pos"][ok] = geom[ok, :3]; out["normal"][ok] = geom[ok, 3:6]; out["min_dist"][ok] = geom[ok, 6]; out["max_dist"][ok] = geom[ok, 7]
    return out
