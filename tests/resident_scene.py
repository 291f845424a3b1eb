"""LastFrame entry lists with known fates for the device-built projection queries (k_track_queries, dvm_track_finish_batch_resident), and
the loop header of SearchByProjection(CurrentFrame, LastFrame) (ORBmatcher.cc:1573-1611) restated in numpy float32, operation for
operation as csrc/pose_f32.h and host/orb_matcher.cpp write it.  No GPU needed."""
import numpy as np
from scipy.spatial.transform import Rotation

K = np.array([500.0, 470.0, 320.0, 240.0], np.float32)       # fx != fy
BOUNDS = np.array([0, 640, 0, 480], np.float32)
NLEVELS = 8
SCALE = (np.float32(1.2) ** np.arange(NLEVELS)).astype(np.float32)
INV_S2 = (1.0 / (SCALE.astype(np.float64) ** 2)).astype(np.float32)
FATES = ("kept", "behind", "left", "right", "above", "below")

LOCAL_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"), ("max_dist", "<f4"), ("desc", "u1", (32,)),
                              ("n_obs", "<i4"), ("bad", "<i4")])


def pose(seed):
    """A predicted Tcw as dvm_se3f (qx qy qz qw tx ty tz), away from the identity."""
    rng = np.random.default_rng(seed)
    q = Rotation.from_rotvec(rng.normal(0, 0.15, 3)).as_quat()
    if q[3] < 0:
        q = -q
    return np.concatenate([q, rng.normal(0, 0.4, 3)]).astype(np.float32)


def entries(n, mode, seed, Tcw=None, store_cap=None):
    """n entries and the records behind them.  mode: 'all' (every entry projects inside), 'none' (every entry fails one gate), 'mix' (about a
    fifth -- 17 % -- fails each gate: behind the camera, left, right, above, below; the rest, 15 %, is kept).  Returns dict(slot, octave, angle, Tcw_pred,
    records [store_cap], fate [n]); records are indexed by slot (a permutation, so that entry order is not slot order)."""
    rng = np.random.default_rng(seed)
    Tcw = pose(seed + 1) if Tcw is None else np.asarray(Tcw, np.float32)
    cap = max(n, 1) if store_cap is None else store_cap
    if mode == "all":
        fate = np.zeros(n, np.int32)
    elif mode == "none":
        fate = rng.integers(1, 6, n).astype(np.int32)
    else:
        fate = rng.choice(6, n, p=[0.15, 0.17, 0.17, 0.17, 0.17, 0.17]).astype(np.int32)
    z = rng.uniform(2.0, 9.0, n)
    u = rng.uniform(20, 620, n); v = rng.uniform(20, 460, n)
    z = np.where(fate == 1, -z, z)
    u = np.where(fate == 2, rng.uniform(-300, -5, n), u); u = np.where(fate == 3, rng.uniform(645, 900, n), u)
    v = np.where(fate == 4, rng.uniform(-300, -5, n), v); v = np.where(fate == 5, rng.uniform(485, 800, n), v)
    Xc = np.column_stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z])
    R = Rotation.from_quat(Tcw[:4].astype(np.float64)).as_matrix()
    Xw = (Xc - Tcw[4:7].astype(np.float64)[None, :]) @ R          # R^T (Xc - t)
    slot = rng.permutation(cap)[:n].astype(np.int32)
    rec = np.zeros(cap, LOCAL_POINT_DTYPE)
    rec["pos"] = rng.normal(0, 1, (cap, 3)).astype(np.float32)
    rec["desc"] = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    rec["n_obs"] = np.where(rng.random(cap) < 0.25, 0, rng.integers(1, 5, cap))       # some entries have n_obs == 0
    rec["pos"][slot] = Xw.astype(np.float32)
    octave = rng.integers(0, NLEVELS, n).astype(np.uint8)
    if n >= 2:
        octave[0], octave[-1] = 0, NLEVELS - 1                                        # octaves 0 and nlevels - 1 are present
    angle = rng.uniform(0, 360, n).astype(np.float32)
    return dict(slot=slot, octave=octave, angle=angle, Tcw_pred=Tcw, records=rec, fate=fate)


def quat_rotate_f32(q, p):
    """dvm_pose::quat_rotate: p + w (2 q x p) + q x (2 q x p), every operation one float32 rounding"""
    q = np.asarray(q, np.float32); p = np.asarray(p, np.float32)
    a0 = q[1] * p[:, 2] - q[2] * p[:, 1]; a1 = q[2] * p[:, 0] - q[0] * p[:, 2]; a2 = q[0] * p[:, 1] - q[1] * p[:, 0]
    a0 = a0 + a0; a1 = a1 + a1; a2 = a2 + a2
    b0 = q[1] * a2 - q[2] * a1; b1 = q[2] * a0 - q[0] * a2; b2 = q[0] * a1 - q[1] * a0
    return np.column_stack([(p[:, 0] + q[3] * a0) + b0, (p[:, 1] + q[3] * a1) + b1, (p[:, 2] + q[3] * a2) + b2]).astype(np.float32)


def loop_header_numpy(e, th, K=K, bounds=BOUNDS, scale=SCALE, project=None):
    """The queries of the entry lists `e` (entries()): dict(nq, q_entry, qx, qy, qr, qmin, qmax, q_claims, q_angle, q_pos, qdesc).
    project(xc, yc, zc) -> (u, v) float32 replaces the pinhole projection (a KannalaBrandt8 restatement)."""
    T = np.asarray(e["Tcw_pred"], np.float32)
    rec = e["records"][e["slot"]]
    X = rec["pos"].astype(np.float32).reshape(-1, 3)
    Xc = quat_rotate_f32(T[:4], X) + T[4:7][None, :]
    xc, yc, zc = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        invzc = (1.0 / zc.astype(np.float64)).astype(np.float32)
        if project is None:
            u = K[0] * xc / zc + K[2]; v = K[1] * yc / zc + K[3]
        else:
            u, v = project(xc, yc, zc)
    keep = ~(invzc < 0) & ~((u < bounds[0]) | (u > bounds[1])) & ~((v < bounds[2]) | (v > bounds[3]))
    i = np.flatnonzero(keep).astype(np.int32)
    octv = e["octave"][i].astype(np.int32)
    return dict(nq=len(i), q_entry=i, qx=u[i].astype(np.float32), qy=v[i].astype(np.float32), qr=(np.float32(th) * scale[octv]).astype(np.float32),
                qmin=octv - 1, qmax=octv + 1, q_claims=(rec["n_obs"][i] > 0).astype(np.uint8), q_angle=e["angle"][i], q_pos=rec["pos"][i],
                qdesc=rec["desc"][i])


QUERY_FIELDS = ("q_entry", "qx", "qy", "qr", "qmin", "qmax", "q_claims", "q_angle", "q_pos", "qdesc")


def assert_queries_equal(a, b, skip=()):
    assert a["nq"] == b["nq"], (a["nq"], b["nq"])
    for k in QUERY_FIELDS:
        if k in skip:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
