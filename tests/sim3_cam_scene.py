"""Scenes and the float64 restatement for the two Sim3 steps on a camera model per keyframe: dvm_sim3_hypotheses_cam (Sim3Solver's
CheckInliers with pCamera1 / pCamera2->project) and dvm_optimize_sim3_cam (Optimizer::OptimizeSim3 whose two edges project with
pCamera1 / pCamera2).  The oracle has no fisheye model, so this file is the reference of tests/test_sim3_cam_scene.py (CPU: what the
scenes contain, the restatement against the oracle on pinhole cameras), tests/test_gpu_sim3_cam.py and tests/test_gpu_kb8_merge.py:

  inliers_cam_f64      sim3_scene.inliers_f64 with each side's projection by its model (KannalaBrandt8: kb8_scene.project_exact)
  optimize_sim3_f64    g2o's Levenberg loop of OptimizeSim3 as oracle/ba_oracle.cpp and k_optimize_sim3 state it -- lambda from the
                       largest diagonal entry, Huber with delta = float(sqrt(th2)), optimize(5), chi2 <= th2 with the kernels off,
                       optimize(5 | 10), the early return below 10 survivors -- with central differences at 1e-9.  On a KannalaBrandt8
                       side the residual and every chi2 test take kb8_scene.project_f64 (the reference's project(Vector3d): float
                       theta; `nudge` moves it by -1 / 0 / +1 float ulp on every edge) and the differences kb8_scene.project_exact
  hyp_scene            sim3_scene.scene with the lateral spread widened: theta up to 1.35 rad in camera 2 and beyond pi / 2 in camera 1,
                       a point on camera 2's optical axis, one with z = 0 and one with z < 0
  sim3_case_cam        sim3_scene.sim3_case through two camera models, theta up to 1.3 rad (0.8 next to a pinhole camera)
  two_agent_scene_kb8  merge_scene.make_two_agent_scene seen through the robot's fisheye camera by both agents

Measured on the CPU (tests/test_sim3_cam_scene.py asserts that both still hold; docs/NOTEBOOK.md lists every case):
  * optimize_sim3_f64 with two pinhole models against oracle.optimize_sim3 over sim3_scene.OPT_CASES: identical masks and counts,
    max |S - S_oracle| = ORACLE_S_DIFF (case ORACLE_S_DIFF_CASE), below RESTATEMENT_GATE = 1e-7 (a tenth of the device's gate against
    the oracle, so the two gates nest);
  * the largest |S(nudge) - S(0)| over the stable fisheye cases = THETA_ULP_S_DIFF (case THETA_ULP_S_DIFF_CASE).  The device's atan2f may
    differ from libm's in the last bit, so the GPU test allows S_BOUND = 10 x that (the project's rule for a theta-quantised residual)."""
import functools

import numpy as np

import sim3_scene as ss
from kb8_scene import ROBOMASTER, TUM, project_exact, project_f32, project_f64

PINHOLE, KB8 = 0, 1
RESTATEMENT_GATE = 1e-7
ORACLE_S_DIFF, ORACLE_S_DIFF_CASE = 6.54e-8, "n255"
THETA_ULP_S_DIFF, THETA_ULP_S_DIFF_CASE = 2.951e-4, "n257"   # (every other case: 1e-5 or less; this one's un-nudged run takes another LM path)
S_BOUND = 10 * THETA_ULP_S_DIFF
UNSTABLE_CASE = None                                     # the one named case allowed to be unstable (not compared on the device): none is


def pinhole(K):
    return (PINHOLE, tuple(float(x) for x in np.asarray(K, np.float32)) + (0.0,) * 4)


def kb8(p):
    return (KB8, tuple(float(x) for x in np.asarray(p, np.float32)))


RM, TM = kb8(ROBOMASTER), kb8(TUM)
PIN = pinhole(ss.K2)      # the wider of sim3_scene's two pinhole cameras: it still sees a part of what a fisheye camera sees
PAIRS = {"rm_tum": (RM, TM), "tum_rm": (TM, RM), "pin_tum": (PIN, TM), "rm_pin": (RM, PIN)}


def params(m):
    return np.asarray(m[1], np.float32)


def camera_model(capi, m):
    """The capi.CameraModel of a model tuple."""
    return capi.CameraModel.make(m[0], m[1])


def as_pinhole(m):
    """The pinhole model of the same fx, fy, cx, cy."""
    return (PINHOLE, tuple(m[1][:4]) + (0.0,) * 4)


def project_model(m, X, mode="exact", nudge=None):
    """Pixels [n, 2] of camera-frame points under model m, float64.  mode "exact": the smooth projection (double atan2); "f64": the
    reference's project(Vector3d) (float theta, `nudge` in float ulps); "f32": project(Vector3f).  A pinhole camera has one formula."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    p = params(m)
    if m[0] == PINHOLE:
        K = p.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], axis=1)
    if mode == "f64":
        return project_f64(p, X, nudge)
    if mode == "f32":
        return project_f32(p, X).astype(np.float64)
    return project_exact(p, X)


def theta(X):
    X = np.asarray(X, np.float64).reshape(-1, 3)
    return np.arctan2(np.hypot(X[:, 0], X[:, 1]), X[:, 2])


# ---- Sim3Solver
HYP_N = (3, 63, 64, 65, 127, 257)
HYP_H = 50
AXIS, Z0, BEHIND = 0, 1, 2        # indices of the special points of a hyp_scene with N >= 63


@functools.lru_cache(maxsize=None)
def hyp_scene(seed=0, N=65, angle=0.3, scale=1.0, outlier_frac=0.1, noise=0.05):
    """(sc, gt) as sim3_scene.scene, without K1 / K2 (the cameras are the test's models).  Camera 2 sees the points over a cone of 1.35 rad
    at depth 3 .. 9; camera 1 is turned by `angle` about its own centre and moved a little, so its thetas pass pi / 2.  With N >= 63, point
    AXIS lies on camera 2's optical axis, point Z0 in its principal plane (z == 0) and point BEHIND behind it (theta = 1.8)."""
    rng = np.random.default_rng([seed, N, 77] + [int(x) for x in np.frombuffer(np.float64([angle, scale]).tobytes(), np.uint32)])
    th = 1.35 * np.sqrt(rng.uniform(0.0, 1.0, N))
    th[-1] = 1.35
    psi = rng.uniform(-np.pi, np.pi, N)
    d = rng.uniform(3.0, 9.0, N)
    P2 = np.column_stack([d * np.sin(th) * np.cos(psi), d * np.sin(th) * np.sin(psi), d * np.cos(th)])
    if N >= 63:
        P2[AXIS] = [0.0, 0.0, 5.0]
        P2[Z0] = [4.0 * np.cos(0.7), 4.0 * np.sin(0.7), 0.0]
        P2[BEHIND] = [6.0 * np.sin(1.8) * np.cos(-2.0), 6.0 * np.sin(1.8) * np.sin(-2.0), 6.0 * np.cos(1.8)]
    axis = rng.normal(size=3)
    axis[2] = 0.0                                     # camera 1 is turned sideways: what is central in one camera is wide in the other
    R = ss.rot(axis, angle)
    t = scale * np.array([0.3, -0.2, 0.5])
    e1 = ss._bounds(rng, N)
    e2 = ss._bounds(rng, N)
    sigma = noise * np.sqrt(np.minimum(e1, e2) / 9.0)
    P1 = scale * (P2 @ R.T) + t + scale * sigma[:, None] * rng.normal(0, 1.0, (N, 3))
    bad = rng.random(N) < outlier_frac
    bad[:3] = False
    P1[bad] += scale * rng.normal(0, 1.0, (int(bad.sum()), 3))
    sc = dict(P1c=P1.astype(np.float32), P2c=P2.astype(np.float32), max_err1=e1, max_err2=e2)
    return ss._freeze(sc), ss._freeze(dict(s=scale, R=R, t=t, bad=bad))


# Per pair, how far camera 1 is turned and the noise (see sim3_scene.scene).  Next to a pinhole camera, whose errors grow with 1 / cos^2(theta),
# the noise is halved and camera 1 turned by 0.9 rad: the points the pinhole camera sees well are then wide in the fisheye camera, so
# the fisheye side's model decides (SWAP_SHARE_MIN).  N = 3 has no special points and no statistics.
HYP_KW = {"rm_tum": dict(angle=0.3, noise=0.02), "tum_rm": dict(angle=0.3, noise=0.02), "pin_tum": dict(angle=0.9, noise=0.01),
          "rm_pin": dict(angle=0.9, noise=0.01)}


def hyp_case(pair, N):
    """(sc, gt, tri, models) of a pair of cameras at N points: HYP_H minimal sets."""
    sc, gt = hyp_scene(0, N, **HYP_KW[pair])
    return sc, gt, ss.triples(0, N, HYP_H), PAIRS[pair]


def inliers_cam_f64(T, sc, models):
    """sim3_scene.inliers_f64 with camera 1 = models[0] and camera 2 = models[1]: (err1, err2) [H, N] in float64."""
    s, R, t = ss.unpack(T)
    P1, P2 = sc["P1c"].astype(np.float64), sc["P2c"].astype(np.float64)
    H, N = len(s), len(P1)
    X21 = s[:, None, None] * np.einsum("hrc,nc->hnr", R, P2) + t[:, None]
    X12 = np.einsum("hcr,hnc->hnr", R, P1[None] - t[:, None]) / s[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e1 = ((project_model(models[0], P1)[None] - project_model(models[0], X21).reshape(H, N, 2)) ** 2).sum(axis=-1)
        e2 = ((project_model(models[1], X12).reshape(H, N, 2) - project_model(models[1], P2)[None]) ** 2).sum(axis=-1)
    return e1, e2


def hyp_reference(sc, tri, fix_scale, models):
    """The restatement alone on a scene: horn_f64 on the minimal sets, then (T [H, 13], inlier, clear, gap_ok [H])."""
    s, R, t, gap = ss.horn_f64(sc["P1c"][tri], sc["P2c"][tri], fix_scale)
    T = np.concatenate([s[:, None], R.reshape(-1, 9), t], axis=1)
    inl, clear = ss.decide(*inliers_cam_f64(T, sc, models), sc)
    return T, inl, clear, gap > ss.GAP_MIN


# ---- OptimizeSim3
def _quat_to_R(q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _R_to_quat(R):
    """Eigen's quaternion from a matrix, (x, y, z, w)."""
    q = np.zeros(4)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t; q[j] = (R[j, i] + R[i, j]) * t; q[k] = (R[k, i] + R[i, k]) * t
    return q


def _sim3_exp(u):
    """g2o::Sim3(Vector7d) (sim3.h:62-125): (q, t, s)."""
    om, up, sigma = np.asarray(u[:3], np.float64), np.asarray(u[3:6], np.float64), float(u[6])
    th = float(np.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]))
    O = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    O2 = O @ O
    I = np.eye(3)
    s = float(np.exp(sigma))
    eps = 0.00001
    if abs(sigma) < eps:
        C = 1.0
        if th < eps:
            A, B = 0.5, 1.0 / 6.0
            R = I + O + O2
        else:
            th2 = th * th
            A = (1 - np.cos(th)) / th2; B = (th - np.sin(th)) / (th2 * th)
            R = I + np.sin(th) / th * O + (1 - np.cos(th)) / (th * th) * O2
    else:
        C = (s - 1) / sigma
        if th < eps:
            s2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / s2; B = ((0.5 * s2 - sigma + 1) * s) / (s2 * sigma)
            R = I + O + O2
        else:
            R = I + np.sin(th) / th * O + (1 - np.cos(th)) / (th * th) * O2
            a, b, th2, s2 = s * np.sin(th), s * np.cos(th), th * th, sigma * sigma
            c = th2 + s2
            A = (a * sigma + (1 - b) * th) / (th * c)
            B = (C - ((b - 1) * sigma + a * th) / c) * 1.0 / th2
    W = A * O + B * O2 + C * I
    return _R_to_quat(R), W @ up, s


def _sim3_mul(a, b):
    p, q = a[0], b[0]
    o = np.array([p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1], p[3] * q[1] + p[1] * q[3] + p[2] * q[0] - p[0] * q[2],
                  p[3] * q[2] + p[2] * q[3] + p[0] * q[1] - p[1] * q[0], p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2]])
    return o, a[2] * (_quat_to_R(a[0]) @ b[1]) + a[1], a[2] * b[2]


def _sim3_inv(a):
    q = np.array([-a[0][0], -a[0][1], -a[0][2], a[0][3]])
    return q, _quat_to_R(q) @ ((-1.0 / a[2]) * a[1]), 1.0 / a[2]


def _sim3_map(S, X):
    R = _quat_to_R(S[0])
    rx = np.stack([R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1] + R[i, 2] * X[:, 2] for i in range(3)], axis=1)
    return S[2] * rx + S[1]


def _robustify(e, delta):
    """(rho0, rho1) of g2o's Huber kernel on chi2 values e [n]; delta [n], 0 where the kernel is off."""
    big = (delta > 0) & (e > delta * delta)
    sq = np.sqrt(np.where(big, e, 1.0))
    return np.where(big, 2 * sq * delta - delta * delta, e), np.where(big, delta / sq, 1.0)


def optimize_sim3_f64(S0, fix_scale, P1, P2, obs1, obs2, w1, w2, models, th2, nudge=0):
    """Optimizer::OptimizeSim3 (Optimizer.cc:1960-2212) on two camera models: (S [8], inlier [N] uint8, nIn).  See the file header."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    obs1, obs2, w1, w2 = (np.asarray(a, np.float64) for a in (obs1, obs2, w1, w2))
    S0 = np.asarray(S0, np.float64)
    N = len(P1)
    S = (S0[:4].copy(), S0[4:7].copy(), float(S0[7]))
    huber = float(np.float32(np.sqrt(np.float32(th2))))
    alive, robust = np.ones(N, bool), np.ones(N, bool)
    chi12, chi21 = np.zeros(N), np.zeros(N)
    DMAX = np.finfo(np.float64).max

    def errors(Sx, idx, mode):
        nd = None if (nudge == 0 or mode != "f64") else np.full(len(idx), nudge)
        a = obs1[idx] - project_model(models[0], _sim3_map(Sx, P2[idx]), mode, nd)
        b = obs2[idx] - project_model(models[1], _sim3_map(_sim3_inv(Sx), P1[idx]), mode, nd)
        return a, b

    def chi_all(Sx):
        idx = np.flatnonzero(alive)
        a, b = errors(Sx, idx, "f64")
        chi12[idx] = w1[idx] * (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]); chi21[idx] = w2[idx] * (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1])
        dl = np.where(robust[idx], huber, 0.0)
        return float(np.sum(_robustify(chi12[idx], dl)[0] + _robustify(chi21[idx], dl)[0])), a, b

    def optimize(iters):
        nonlocal S
        lam, ni, nbad = -1.0, 2.0, 0
        for it in range(iters):
            cur, e12, e21 = chi_all(S)
            ini = cur
            idx = np.flatnonzero(alive)
            J12, J21 = np.zeros((len(idx), 2, 7)), np.zeros((len(idx), 2, 7))
            for d in range(7):
                u = np.zeros(7); u[d] = 1e-9
                if fix_scale:
                    u[6] = 0
                ap, bp = errors(_sim3_mul(_sim3_exp(u), S), idx, "exact")
                u = np.zeros(7); u[d] = -1e-9
                if fix_scale:
                    u[6] = 0
                am, bm = errors(_sim3_mul(_sim3_exp(u), S), idx, "exact")
                J12[:, :, d] = 5e8 * (ap - am); J21[:, :, d] = 5e8 * (bp - bm)
            H, b = np.zeros((7, 7)), np.zeros(7)
            dl = np.where(robust[idx], huber, 0.0)
            for J, e, w0 in ((J12, e12, w1[idx]), (J21, e21, w2[idx])):
                r1 = _robustify(w0 * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]), dl)[1]
                H += np.einsum("n,nra,nrc->ac", r1 * w0, J, J)
                b += np.einsum("nra,nr->a", J, -(w0 * r1)[:, None] * e)
            if it == 0:
                lam, ni, nbad = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                bak = S
                x = None
                try:
                    L = np.linalg.cholesky(H + lam * np.eye(7))
                    x = np.linalg.solve(L.T, np.linalg.solve(L, b))
                except np.linalg.LinAlgError:
                    x = None
                if x is None:
                    temp, scale = DMAX, 0.0
                else:
                    u = x.copy()
                    if fix_scale:
                        u[6] = 0
                    S = _sim3_mul(_sim3_exp(u), S)
                    temp = chi_all(S)[0]
                    scale = float(np.sum(x * (lam * x + b)))
                rho = (cur - temp) / (scale + 1e-3)
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha); ni = 2.0; cur = temp
                else:
                    lam *= ni; ni *= 2; S = bak
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                break
            nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
            if nbad >= 3:
                break

    optimize(5)
    badm = (chi12 > th2) | (chi21 > th2)
    alive[badm] = False
    robust[~badm] = False
    inlier = np.zeros(N, np.uint8)
    nbad_total = int(badm.sum())
    if N - nbad_total < 10:
        return S0.copy(), inlier, 0
    optimize(10 if nbad_total > 0 else 5)
    idx = np.flatnonzero(alive)
    a, b = errors(S, idx, "f64")
    c12 = w1[idx] * (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]); c21 = w2[idx] * (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1])
    inlier[idx[~((c12 > th2) | (c21 > th2))]] = 1
    return np.r_[S[0], S[1], S[2]], inlier, int(inlier.sum())


def chi2_cam_f64(S, P1, P2, obs1, obs2, w1, w2, models):
    """(chi12, chi21) [N] of the two edges at S = (q, t, s) through the reference's project(Vector3d) of each model."""
    Sx = (np.asarray(S[:4], np.float64), np.asarray(S[4:7], np.float64), float(S[7]))
    a = np.asarray(obs1, np.float64) - project_model(models[0], _sim3_map(Sx, np.asarray(P2, np.float64)), "f64")
    b = np.asarray(obs2, np.float64) - project_model(models[1], _sim3_map(_sim3_inv(Sx), np.asarray(P1, np.float64)), "f64")
    return np.asarray(w1) * (a ** 2).sum(axis=1), np.asarray(w2) * (b ** 2).sum(axis=1)


@functools.lru_cache(maxsize=None)
def sim3_case_cam(seed, N=150, out_frac=0.1, fix_scale=False, noise=0.6, gross=(), s0_scale=None, pair="rm_tum"):
    """(S0, P1, P2, obs1, obs2, w1, w2) for optimize_sim3_cam on the models PAIRS[pair], as sim3_scene.sim3_case lays it out: the points
    over a cone of 1.3 rad in camera 2 (0.8 rad when one of the cameras is a pinhole camera, whose projection ends at pi / 2), depth 4 .. 12,
    observed through each model's project(Vector3d) plus `noise` px; gross and random outliers as there.  Read-only (cached)."""
    from dvm_slam_amd.synth import _quat_from_rot, _rot_from_axis_angle
    m1, m2 = PAIRS[pair]
    rng = np.random.default_rng([seed, 4242])
    R = ss.rot(rng.normal(size=3), rng.uniform(-0.3, 0.3))
    t = rng.uniform(-0.5, 0.5, 3)
    s = 1.0 if fix_scale else rng.uniform(0.7, 1.4)
    if fix_scale and s0_scale is not None:
        s = float(s0_scale)
    cone = 1.3 if (m1[0] == KB8 and m2[0] == KB8) else 0.8
    th = cone * np.sqrt(rng.uniform((0.02 / cone) ** 2, 1.0, N))
    th[0] = cone
    psi = rng.uniform(-np.pi, np.pi, N)
    d = rng.uniform(4.0, 12.0, N)
    P2 = np.column_stack([d * np.sin(th) * np.cos(psi), d * np.sin(th) * np.sin(psi), d * np.cos(th)])
    P1 = (s * (R @ P2.T)).T + t
    obs1 = project_model(m1, P1, "f64") + rng.normal(0, 1.0, (N, 2)) * noise
    obs2 = project_model(m2, P2, "f64") + rng.normal(0, 1.0, (N, 2)) * noise
    bad = rng.random(N) < out_frac
    obs1[bad] += rng.choice([-1, 1], (int(bad.sum()), 2)) * 25.0
    gross = np.asarray(gross, np.int64)
    obs1[gross] += 80.0 * ss._SIGNS[np.arange(len(gross)) % 4]
    w1 = 1.2 ** (-2.0 * rng.integers(0, 8, N)); w2 = 1.2 ** (-2.0 * rng.integers(0, 8, N))
    R0 = _rot_from_axis_angle(rng.normal(0, 0.01, 3)) @ R
    s0 = float(s0_scale) if s0_scale is not None else s * (1.0 if fix_scale else 1.05)
    S0 = np.r_[_quat_from_rot(R0), t + rng.normal(0, 0.02, 3), s0]
    out = (S0, P1, P2, obs1, obs2, w1, w2)
    for a in out:
        a.setflags(write=False)
    return out


_EVEN = tuple(range(0, 20, 2))
# the cases of sim3_scene.OPT_CASES on fisheye cameras, the swapped pair and the two mixed pairs
OPT_CASES_CAM = {
    "n10": dict(kw=dict(seed=10, N=10, out_frac=0.0), th2=10.0, survivors=10, second_round=5),
    "n255": dict(kw=dict(seed=255, N=255), th2=10.0, survivors=None, second_round=10),
    "n256": dict(kw=dict(seed=256, N=256), th2=10.0, survivors=None, second_round=10),
    "n257": dict(kw=dict(seed=257, N=257), th2=10.0, survivors=None, second_round=10),
    "n513": dict(kw=dict(seed=513, N=513), th2=10.0, survivors=None, second_round=10),
    "n257_swapped": dict(kw=dict(seed=257, N=257, pair="tum_rm"), th2=10.0, survivors=None, second_round=10),
    "n257_pin_tum": dict(kw=dict(seed=257, N=257, pair="pin_tum"), th2=10.0, survivors=None, second_round=10),
    "n257_rm_pin": dict(kw=dict(seed=257, N=257, pair="rm_pin"), th2=10.0, survivors=None, second_round=10),
    "survive9": dict(kw=dict(seed=40, N=20, out_frac=0.0, noise=0.0, gross=_EVEN + (1,)), th2=10.0, survivors=9, second_round=0),
    "survive10": dict(kw=dict(seed=40, N=20, out_frac=0.0, noise=0.0, gross=_EVEN), th2=10.0, survivors=10, second_round=10),
    "survive11": dict(kw=dict(seed=40, N=20, out_frac=0.0, noise=0.0, gross=_EVEN[:9]), th2=10.0, survivors=11, second_round=10),
    "clean": dict(kw=dict(seed=50, N=60, out_frac=0.0, noise=0.0), th2=10.0, survivors=60, second_round=5),
    "gross3": dict(kw=dict(seed=51, N=60, out_frac=0.0, noise=0.0, gross=(3, 17, 40)), th2=10.0, survivors=57, second_round=10),
    "fix_scale_1.3": dict(kw=dict(seed=52, N=100, fix_scale=True, s0_scale=1.3), th2=10.0, survivors=None, second_round=10),
    "th2_10": dict(kw=dict(seed=53, N=150), th2=10.0, survivors=None, second_round=10),
    "th2_25": dict(kw=dict(seed=53, N=150), th2=25.0, survivors=None, second_round=10),
}


def opt_case_cam(name):
    """(case tuple of sim3_case_cam, fix_scale, th2, spec, models) of OPT_CASES_CAM[name]."""
    spec = OPT_CASES_CAM[name]
    return sim3_case_cam(**spec["kw"]), bool(spec["kw"].get("fix_scale", False)), spec["th2"], spec, PAIRS[spec["kw"].get("pair", "rm_tum")]


@functools.lru_cache(maxsize=None)
def opt_reference(name, nudge=0):
    """(S, inlier, nIn) of optimize_sim3_f64 on a case, computed once."""
    (S0, *rest), fix, th2, spec, models = opt_case_cam(name)
    S, inl, n = optimize_sim3_f64(S0, fix, *rest, models, th2, nudge)
    S.setflags(write=False); inl.setflags(write=False)
    return S, inl, n


def is_stable(name):
    ref = opt_reference(name)
    return all(np.array_equal(opt_reference(name, nd)[1], ref[1]) and opt_reference(name, nd)[2] == ref[2] for nd in (-1, 1))


def theta_ulp_s_diff():
    """The measurement behind THETA_ULP_S_DIFF: {case: max |S(nudge) - S(0)| over nudge = -1, +1} for the stable cases that run a second round."""
    out = {}
    for name, spec in OPT_CASES_CAM.items():
        if spec["second_round"] == 0 or not is_stable(name):
            continue
        S = opt_reference(name)[0]
        out[name] = max(float(np.abs(opt_reference(name, nd)[0] - S).max()) for nd in (-1, 1))
    return out


# ---- the merge flow on a fisheye two-agent scene
def two_agent_scene_kb8(oracle, seed=0, n_distract=4):
    """merge_scene.make_two_agent_scene (about 1 100 points, one true candidate among n_distract distractors) as two robots with the
    fisheye camera see it: every keypoint's pinhole ray is projected through ROBOMASTER (mvKeysUn = mvKeys), K = p[0..3] and the bounds
    of the 960 x 540 image.  The returned dict adds models = (RM, RM)."""
    from merge_scene import make_two_agent_scene
    sc = make_two_agent_scene(oracle, seed, n_distract=n_distract)
    bounds = np.array([0.0, 960.0, 0.0, 540.0], np.float32)

    def through_fisheye(kf):
        K = kf["K"].astype(np.float64)
        kps = kf["kps"].copy()
        ray = np.column_stack([(kps["x"].astype(np.float64) - K[2]) / K[0], (kps["y"].astype(np.float64) - K[3]) / K[1], np.ones(len(kps))])
        uv = project_exact(ROBOMASTER, ray)
        kps["x"] = uv[:, 0]; kps["y"] = uv[:, 1]
        return dict(kf, kps=kps, K=ROBOMASTER[:4].copy(), bounds=bounds)
    return dict(sc, a=through_fisheye(sc["a"]), peers=[through_fisheye(p) for p in sc["peers"]], models=(RM, RM))
