"""Scenes for dvm_pose_optimize / dvm_pose_pool_optimize (k_pose_optimize: Optimizer::PoseOptimization, Optimizer.cc:744-1028) with
fx != fy, at sizes on both sides of the 1 280 correspondences a workgroup keeps in registers, and pose_f64: a plain numpy float64
restatement of PoseOptimization over g2o's Levenberg (optimization_algorithm_levenberg.cpp:59-165), written from those two sources, which
also counts what a scene contains (trials, failed solves, rounds ending on a rejected trial, re-admitted edges on either side of index
1 280, rounds without an active edge, the distance of every classified chi2 from 5.991).  tests/test_oracle_pose.py pins the oracle to
it on the CPU and asserts what the scenes hold; tests/test_gpu_pose.py runs the device on the same tables."""
import functools

import numpy as np

K_DEFAULT = (520.0, 390.0, 300.0, 250.0)       # fx / fy = 1.33: a projection row taken with the other focal length moves by a third
K_SWAPPED = (390.0, 520.0, 250.0, 300.0)
K_SUITE = (149.0, 149.0, 320.0, 240.0)         # synth.FX == synth.FY, what every other pose test runs on
REG = 1280                                      # kPoseEdgesPerThread x 256: edges from this index on live in global memory on the device
CHI2_MONO = np.float32(5.991)
BAND_MIN = 1e-4         # every classified chi2 of a case compared flag for flag lies at least this far (relative) from 5.991
SWAP_SHARE_MIN = 0.30   # exchanging fx and fy (or cx and cy) must change at least this share of a scene's flags
TAIL_OUTLIERS_MIN = 20  # planted outliers at index >= 1 280 for N >= 1 537
READMIT_MIN = 3         # re-admitted edges below, and at or above, index 1 280 in the scenes named for it

# Largest deviation of the oracle from pose_f64 over every case of the tables below, measured on the CPU (docs/NOTEBOOK.md section 15
# lists the cases): max |t - t64| and max |q - q64| of the returned pose.  The CPU test asserts 4 x these.
ORACLE_DT_MAX, ORACLE_DQ_MAX = 4.67e-10, 1.22e-11
BOUND_DT, BOUND_DQ = 4 * ORACLE_DT_MAX, 4 * ORACLE_DQ_MAX


def quat_to_R(q):
    """(x, y, z, w) of unit norm -> R."""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat(R):
    """Eigen's quaternion from a rotation matrix, (x, y, z, w)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.empty(4)
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
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def normalize_pose(pose):
    """(t, q) with q as SE3Quat::normalizeRotation leaves it: w >= 0, unit norm."""
    p = np.array(pose, np.float64)
    if p[6] < 0:
        p[3:] = -p[3:]
    p[3:] /= np.sqrt((p[3:] ** 2).sum())
    return p


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def _rodrigues(om):
    """(R, V) of SE3Quat::exp (se3quat.h:212-240)."""
    th = np.sqrt(om @ om)
    O = _skew(om)
    O2 = O @ O
    if th < 0.00001:
        R = np.eye(3) + O + O2
        return R, R
    s, c = np.sin(th), np.cos(th)
    return np.eye(3) + s / th * O + (1 - c) / (th * th) * O2, np.eye(3) + (1 - c) / (th * th) * O + (th - s) / (th ** 3) * O2


def oplus(pose, u):
    """VertexSE3Expmap::oplusImpl: exp(u) * pose, u = (omega, upsilon); pose = (t, q)."""
    R, V = _rodrigues(np.asarray(u[:3], np.float64))
    dq = normalize_pose(np.r_[0.0, 0.0, 0.0, R_to_quat(R)])[3:]
    Rd = quat_to_R(dq)
    x1, y1, z1, w1 = dq
    x2, y2, z2, w2 = pose[3:]
    q = np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                  w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
    return normalize_pose(np.r_[V @ np.asarray(u[3:], np.float64) + Rd @ pose[:3], q])


def project(K, Xc):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)


def chi2_f64(pose, Xw, obs, w, K):
    """EdgeSE3ProjectXYZOnlyPose::computeError + chi2() of every edge at `pose`: (chi2 [N], e [N, 2], Xc [N, 3])."""
    Xc = Xw @ quat_to_R(pose[3:]).T + pose[:3]
    with np.errstate(invalid="ignore", over="ignore"):
        e = obs - project(K, Xc)
        return e[:, 0] * w * e[:, 0] + e[:, 1] * w * e[:, 1], e, Xc


def pose_f64(pose, Xw, obs, w, K):
    """Optimizer::PoseOptimization, monocular edges, float64 numpy.  pose = (t, q = (x, y, z, w)); Xw [N, 3]; obs [N, 2]; w = inv_sigma2
    [N]; K = (fx, fy, cx, cy).  Returns (pose [7], outlier [N] uint8, n_inliers, info).

    Four rounds of optimize(10) from the (normalised) input pose, every round over the edges of level 0; Huber with delta =
    float(sqrt(5.991)), taken off after the third round; g2o's Levenberg: lambda0 = 1e-5 max diag H at a round's first iteration,
    rho = (chi - chi') / (x . (lambda x + b) + 1e-3), accepted if rho > 0 and chi' finite with lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3)),
    rejected otherwise with lambda *= ni, ni *= 2 and the state restored; the trial loop ends on rho >= 0 (or NaN) or after 10 trials; the
    round ends on 10 trials, rho == 0, or three iterations in a row that gain less than a thousandth.  A failed 6 x 6 factorisation
    applies no update, evaluates nothing and sets chi' = DBL_MAX (g2o itself applies whatever its solution vector holds from an earlier
    solve, undefined before the first; the oracle and the device define it as no update).  After a round every edge is classified on
    float(chi2) > 5.991f: outliers of the round before recompute their error at the round's final pose, the others report their last
    evaluation -- that of a rejected trial if the round ended on one.  N < 3 returns 0 and the input as given; fewer than 10 edges run
    one round.

    info: rounds; trials (per round, per iteration); failed_solves; rejected_end (rounds that ended on a rejected trial); readmit_lo /
    readmit_hi (edges flagged after a round and cleared after the next, below / from index 1 280); empty_rounds (rounds with no active
    edge); flagged_per_round; min_band (smallest |chi2 / 5.991 - 1| over every classified edge of every round); min_rho (smallest |rho|
    of a trial whose solve succeeded); min_gain (smallest relative distance of (ini - cur) 1e3 from ini)."""
    pose = np.array(pose, np.float64)
    Xw = np.asarray(Xw, np.float64).reshape(-1, 3); obs = np.asarray(obs, np.float64).reshape(-1, 2); w = np.asarray(w, np.float64).ravel()
    fx, fy, cx, cy = (float(v) for v in K)
    N = len(Xw)
    info = dict(rounds=0, trials=[], failed_solves=0, rejected_end=0, readmit_lo=0, readmit_hi=0, empty_rounds=0, flagged_per_round=[],
                min_band=np.inf, min_rho=np.inf, min_gain=np.inf)
    if N < 3:
        return pose, np.zeros(N, np.uint8), 0, info
    delta = float(np.float32(np.sqrt(5.991)))
    T0 = normalize_pose(pose)
    outlier = np.zeros(N, bool)
    last = np.zeros(N)
    robust = True
    DMAX = np.finfo(np.float64).max

    def errors(T, act):
        """computeActiveErrors + activeRobustChi2 over the edges `act`: records their chi2, returns (sum rho, e, Xc, chi2)."""
        c, e, Xc = chi2_f64(T, Xw[act], obs[act], w[act], (fx, fy, cx, cy))
        last[act] = c
        with np.errstate(invalid="ignore", over="ignore"):
            r0 = np.where(c <= delta * delta, c, 2 * np.sqrt(c) * delta - delta * delta) if robust else c
        return float(np.sum(r0)), e, Xc, c

    def system(e, Xc, c, wa):
        """buildSystem: H = sum rho' J^T W J, b = -sum rho' J^T W e, J = -projectJac * [-skew(Xc) | I]."""
        x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        n = len(x)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            r1 = np.where(c <= delta * delta, 1.0, delta / np.sqrt(c)) if robust else np.ones(n)
            Jp = np.zeros((n, 2, 3))
            Jp[:, 0, 0] = -(fx / z); Jp[:, 0, 2] = fx * x / (z * z)
            Jp[:, 1, 1] = -(fy / z); Jp[:, 1, 2] = fy * y / (z * z)
            S = np.zeros((n, 3, 6))
            S[:, 0, 1] = z; S[:, 0, 2] = -y; S[:, 1, 0] = -z; S[:, 1, 2] = x; S[:, 2, 0] = y; S[:, 2, 1] = -x
            S[:, 0, 3] = S[:, 1, 4] = S[:, 2, 5] = 1.0
            J = np.einsum("nij,njk->nik", Jp, S)
            H = np.einsum("n,nia,nib->ab", r1 * wa, J, J)
            b = -np.einsum("n,nia,ni->a", r1 * wa, J, e)
        return H, b

    for rnd in range(4):
        info["rounds"] += 1
        T = T0.copy()
        act = np.flatnonzero(~outlier)
        trials = []
        ended_rejected = False
        if len(act) == 0:
            info["empty_rounds"] += 1
        else:
            lam, ni, nbad = 0.0, 2.0, 0
            for it in range(10):
                cur, e, Xc, c = errors(T, act)
                ini = cur
                H, b = system(e, Xc, c, w[act])
                if it == 0:
                    with np.errstate(invalid="ignore"):
                        lam, ni, nbad = 1e-5 * float(np.max(np.r_[0.0, np.abs(np.diag(H))[np.isfinite(np.diag(H))]])), 2.0, 0
                qmax, rho = 0, 0.0
                while True:
                    bak = T.copy()
                    x = None
                    A = H + lam * np.eye(6)
                    if np.isfinite(A).all() and np.isfinite(b).all():
                        try:
                            L = np.linalg.cholesky(A)
                            x = np.linalg.solve(L.T, np.linalg.solve(L, b))
                        except np.linalg.LinAlgError:
                            x = None
                    if x is None:
                        info["failed_solves"] += 1
                        temp, scale = DMAX, 0.0
                    else:
                        T = oplus(T, x)
                        temp = errors(T, act)[0]
                        scale = float(x @ (lam * x + b))
                    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                        rho = (np.float64(cur) - np.float64(temp)) / np.float64(scale + 1e-3)
                    if x is not None and np.isfinite(rho):
                        info["min_rho"] = min(info["min_rho"], abs(float(rho)))
                    if rho > 0 and np.isfinite(temp):
                        with np.errstate(invalid="ignore", over="ignore"):
                            alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha); ni = 2.0; cur = temp
                        ended_rejected = False
                    else:
                        lam *= ni; ni *= 2; T = bak
                        ended_rejected = x is not None          # the edges now report the errors of a state that was thrown away
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                trials.append(qmax)
                if qmax == 10 or rho == 0:
                    break
                with np.errstate(invalid="ignore", over="ignore"):
                    gain = (ini - cur) * 1e3
                    if np.isfinite(gain) and np.isfinite(ini) and ini > 0:
                        info["min_gain"] = min(info["min_gain"], abs(gain - ini) / ini)
                    nbad = nbad + 1 if gain < ini else 0
                if nbad >= 3:
                    break
        info["trials"].append(trials)
        info["rejected_end"] += int(ended_rejected)
        prev = outlier.copy()
        if prev.any():
            idx = np.flatnonzero(prev)
            last[idx] = chi2_f64(T, Xw[idx], obs[idx], w[idx], (fx, fy, cx, cy))[0]
        with np.errstate(invalid="ignore", over="ignore"):
            outlier = last.astype(np.float32) > CHI2_MONO
            band = np.abs(last / 5.991 - 1.0)
        if np.isfinite(band).any():
            info["min_band"] = min(info["min_band"], float(np.nanmin(band[np.isfinite(band)])))
        back = np.flatnonzero(prev & ~outlier)
        info["readmit_lo"] += int((back < REG).sum()); info["readmit_hi"] += int((back >= REG).sum())
        info["flagged_per_round"].append(int(outlier.sum()))
        if rnd == 2:
            robust = False
        if N < 10:
            break
    return T, outlier.astype(np.uint8), int(N - outlier.sum()), info


# ---- scenes
def _rot(axis, angle):
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = _skew(ax)
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def scene(seed, N, K=K_DEFAULT, out_frac=0.1, shift_px=35.0, noise_px=0.7, pose_noise=(0.003, 0.02), all_out=False, head_out=False):
    """One camera at a known pose, N world points in front of it at depths of 4 to 40 (uniform in inverse depth), spread over a 600 x 500
    image through K = (fx, fy, cx, cy); inv_sigma2 = 1.2^(-2 level) of eight octave levels; noise_px Gaussian on every observation; a share
    out_frac of gross outliers moved by +-shift_px in u and in v with independent signs (all of them with all_out); the edge order
    permuted after the outliers are planted (head_out: instead, exactly the edges below index 1 280 are the outliers, so that from round
    2 on every active edge lies in the part the device keeps in global memory).  The start is the true pose turned by N(0, pose_noise[0]) rad about each axis and moved by
    N(0, pose_noise[1]).  Returns a read-only dict: pose0, Xw, obs, w, K, pose_gt, bad.  The random stream does not depend on K: the same
    seed and N give the same points in the camera frame and the same pixel offsets under every camera."""
    rng = np.random.default_rng([seed, N])
    K = tuple(float(v) for v in K)
    R = _rot(rng.normal(size=3), rng.uniform(-0.5, 0.5))
    t = rng.uniform(-1.0, 1.0, 3)
    z = 1.0 / rng.uniform(1.0 / 40.0, 1.0 / 4.0, N)
    u, v = rng.uniform(-300.0, 300.0, N), rng.uniform(-250.0, 250.0, N)         # offsets from the principal point under the default focal lengths
    Xc = np.column_stack([u / K_DEFAULT[0] * z, v / K_DEFAULT[1] * z, z])
    Xw = (Xc - t) @ R                                                             # R^T (Xc - t)
    obs = project(K, Xc) + rng.normal(0.0, 1.0, (N, 2)) * noise_px
    bad = np.ones(N, bool) if all_out else np.arange(N) < REG if head_out else rng.random(N) < out_frac
    obs[bad] += rng.choice([-1.0, 1.0], size=(int(bad.sum()), 2)) * shift_px
    w = 1.2 ** (-2.0 * rng.integers(0, 8, N))
    perm = np.arange(N) if head_out else rng.permutation(N)
    Xw, obs, w, bad = Xw[perm], obs[perm], w[perm], bad[perm]
    gt = np.r_[t, R_to_quat(R)]
    gt = normalize_pose(gt)
    pose0 = oplus(gt, np.r_[rng.normal(0.0, pose_noise[0], 3), rng.normal(0.0, pose_noise[1], 3)])
    return _freeze(dict(pose0=pose0, Xw=np.ascontiguousarray(Xw), obs=np.ascontiguousarray(obs), w=np.ascontiguousarray(w),
                        K=np.array(K), pose_gt=gt, bad=bad))


def args(sc):
    """(pose, Xw, obs, inv_sigma2, K): the arguments of oracle.pose_optimize, pose_f64 and PosePool.optimize."""
    return sc["pose0"], sc["Xw"], sc["obs"], sc["w"], sc["K"]


def with_K(sc, K):
    """The same arrays called with another camera (not re-projected: the call is wrong on purpose)."""
    return dict(sc, K=np.array(K, np.float64))


def swap_f(sc):
    fx, fy, cx, cy = sc["K"]
    return with_K(sc, (fy, fx, cx, cy))


def swap_c(sc):
    fx, fy, cx, cy = sc["K"]
    return with_K(sc, (fx, fy, cy, cx))


def with_pose(sc, pose):
    return dict(sc, pose0=np.array(pose, np.float64))


def threshold_scene(seed, N, chi2=5.9910002, w=1e-12):
    """Identity pose, noise-free observations, and edge N // 2 with inv_sigma2 = w and its observation moved by sqrt(chi2 / w) in u: with a
    weight of 1e-12 the edge does not move the fit (its pull is 1e-12 of the others'), so its chi2 at the optimum is the one asked for.
    5.9910002 lies between 5.991 and the midpoint above 5.991f = 5.99100018 (float ulp 4.8e-7): float(chi2) > 5.991f is false, the
    double comparison chi2 > 5.991 is true.  The offset is 2.4e6 px, so a pose within 1e-6 (1e-4 px at these depths) moves the value
    by 1e-10 relative, against 3e-8 to either end of the interval."""
    sc = scene(seed, N, out_frac=0.0, noise_px=0.0)
    Xc = sc["Xw"] @ quat_to_R(sc["pose_gt"][3:]).T + sc["pose_gt"][:3]
    obs, ww = sc["obs"].copy(), sc["w"].copy()
    ww[N // 2] = w
    obs[N // 2] = project(sc["K"], Xc[N // 2:N // 2 + 1])[0] + np.array([np.sqrt(chi2 / w), 0.0])
    I = np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    return dict(sc, Xw=Xc, obs=obs, w=ww, pose0=I, pose_gt=I)


def depth0_scene(seed, N, point):
    """Identity pose, noise-free observations of points given in the camera frame, and edge N // 2 replaced by `point` with z == 0 exactly:
    (0.3, -0.2, 0) projects to (+inf, -inf), (0, 0, 0) to (NaN, NaN)."""
    sc = scene(seed, N, out_frac=0.0, noise_px=0.0)
    Xc = sc["Xw"] @ quat_to_R(sc["pose_gt"][3:]).T + sc["pose_gt"][:3]
    Xc[N // 2] = point
    return dict(sc, Xw=Xc, pose0=np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], pose_gt=np.r_[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])


# ---- case tables: name -> keyword arguments of scene().  Seeds: the first of 0, 1, 2, ... whose scene has min_band >= BAND_MIN under
# pose_f64 (tests/test_oracle_pose.py asserts it; docs/NOTEBOOK.md section 15 records the seeds: 0 passed everywhere).
SIZES = {n: dict(seed=0, N=n) for n in (3, 9, 10, 11, 63, 64, 65, 255, 256, 257, 1279, 1280, 1281, 1537, 2561, 4097, 8192)}
CAMERAS = {(name, n): dict(seed=0, N=n, K=K) for n in (300, 1537) for name, K in (("default", K_DEFAULT), ("swapped", K_SWAPPED), ("suite", K_SUITE))}
BATCH_STRIDE = 2600
BATCH = [dict(seed=0, N=n) for n in (2561, 0, 2, 1281, 9, 1280, 300)]
STAGING = dict(seed=0, N=1000)           # test_stride_and_staging: one frame at several strides and inside batches
# Re-admission: 2 to 3 px of noise put hundreds of good edges near 2.45 sigma, and the flagged set moves from round to round (a rough start
# alone does not do it: from 0.05 rad / 0.5 the Levenberg steps reach the optimum inside round 1's ten iterations, from 0.3 rad / 3 they
# either do or end behind the points with every edge flagged -- measured with pose_f64).  Both scenes also end a round on a rejected trial.
READMIT = {"readmit_2000": dict(seed=0, N=2000, noise_px=3.0, pose_noise=(0.05, 0.5)), "readmit_3000": dict(seed=0, N=3000, noise_px=2.0, pose_noise=(0.05, 0.5))}
# rounds that end on a rejected trial (qmax == 10 or rho == 0: the inliers report the errors of a state that was thrown away) and
# iterations of two or more trials, below and above 1 280
REJECTED = {"rejected_1000": dict(seed=0, N=1000), "rejected_4097": dict(seed=0, N=4097)}
ALL_OUT = {"all_out_300": dict(seed=0, N=300, shift_px=80.0, all_out=True), "all_out_1537": dict(seed=0, N=1537, shift_px=80.0, all_out=True)}


# every edge below index 1 280 at +-80 px, the 720 behind them good: rounds 2 to 4 run on tail edges alone
HEAD_OUT = {"head_out_2000": dict(seed=0, N=2000, shift_px=80.0, head_out=True)}


def all_cases():
    """Every named scene compared flag for flag: (name, keyword arguments)."""
    out = [(f"size_{n}", kw) for n, kw in SIZES.items()]
    out += [(f"cam_{name}_{n}", kw) for (name, n), kw in CAMERAS.items()]
    out += [(f"batch_{kw['N']}", kw) for kw in BATCH if kw["N"] >= 3]
    out += [("staging", STAGING)] + list(READMIT.items()) + list(REJECTED.items()) + list(ALL_OUT.items()) + list(HEAD_OUT.items())
    seen, uniq = set(), []
    for name, kw in out:
        key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))
        if key not in seen:
            seen.add(key); uniq.append((name, kw))
    return uniq
