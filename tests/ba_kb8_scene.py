"""Bundle adjustment on a KannalaBrandt8 camera: the reference and the scenes of tests/test_ba_kb8_model.py and tests/test_gpu_ba_kb8.py.
The oracle has no fisheye model, so, as tests/kb8_scene.py does for PoseOptimization, this file restates the solve in numpy float64:

  ba_f64        Optimizer::BundleAdjustment / LocalBundleAdjustment over g2o's Levenberg as oracle/ba_oracle.cpp states it -- lambda_0 =
                1e-5 max |diag H| over camera and landmark blocks, rho = (chi2 - chi2_trial) / (x (lambda x + b) + 1e-3), the cube rule,
                at most 10 trials per iteration, the (ini - cur) 1e3 < ini three-times stop -- with the normal equations solved DENSELY
                ((H + lambda I) x = b by Cholesky: the Schur solve up to rounding) and the camera given as two functions
  pinhole_camera / kb8_camera   those two functions: Pinhole, and kb8_scene.project_f64 (float theta) / project_jac (double theta)
  ba_scene      P cameras a few units apart looking at a cloud 5 to 14 units away, every observation at theta in [0.5 deg, 80 deg]
  ba_case       the first seed whose draw is admissible: the reference and the reference with every edge's theta one float32 ulp off
                ("nudge") take the same trials and stop for the same reason, every final chi2 is far from 5.991, no point near the axis
  theta_ulp_ba_diff   the tolerance: what that ulp moves poses and points by, over all ten admitted scenes

Edges are numpy records (pose, point, u, v, inv_sigma2), the layout of dvm_ba_edge."""
import functools

import numpy as np
import scipy.linalg

import kb8_scene as ks
from pose_scene import normalize_pose, oplus, quat_to_R, R_to_quat, _rot, _freeze

EDGE_DTYPE = np.dtype([("pose", "<i4"), ("point", "<i4"), ("u", "<f8"), ("v", "<f8"), ("inv_sigma2", "<f8")])
CHI2_MONO = 5.991
HUBER = float(np.sqrt(5.991))
ITERATIONS = 10
DMAX = np.finfo(np.float64).max
OUT_SHIFT_PX = 35.0
THETA_MIN, THETA_MAX = np.deg2rad(0.5), np.deg2rad(80.0)
AXIS_MARGIN = 1e-3           # every observation keeps rho >= AXIS_MARGIN |z| (projectJac is 0 / 0 on the axis)
BAND_FACTOR = 10.0           # every final chi2 lies BAND_FACTOR x the scene's largest chi2 difference away from 5.991
MAX_SEEDS = 8
TOL_FACTOR, TOL_FLOOR = 10.0, 1e-6    # the project's margin for results that depend on the last bit (test_gpu_ba_weak.py, kb8_scene.py)
PINHOLE_TOL = 1e-6           # the project's contract between two summation orders of the same recipe (include/dvmslam_hip.h)

# case -> (P, fixed, L, E): the smallest shapes at which k_edge_eval and its dispatch can go wrong
CASES = {
    "a": (4, 2, 32, 127),       # a wave's tail; 2 free cameras (a pinhole problem of this size runs the sequential-order window kernel)
    "b": (6, 2, 48, 256),       # exactly one workgroup
    "c": (6, 2, 48, 257),       # one edge in a second workgroup
    "d": (12, 2, 200, 1471),    # past six free cameras, ragged last wave
    "e": (24, 3, 400, 5003),    # several tiles' worth of edges, multi-block Schur complement
}
MODELS = tuple(ks.MODELS)      # robomaster, tum
PINHOLE_K = (400.0, 380.0, 480.0, 270.0)    # the pinhole camera of the restatement's own check (fx != fy)

# Largest differences between ba_f64 as is and ba_f64 with every edge's theta one float32 ulp off, over the ten admitted scenes of
# all_cases(): measured on the CPU (tests/test_ba_kb8_model.py asserts that theta_ulp_ba_diff() still lies between half of these and
# these; docs/NOTEBOOK.md section 18 lists every scene).  The GPU test allows TOL_FACTOR x the measurement, TOL_FLOOR at least.
THETA_ULP_BA_POSE_DIFF = 9.5e-7      # measured 9.27e-7 (robomaster, case c), recorded rounded up
THETA_ULP_BA_POINT_DIFF = 1.45e-5    # measured 1.40e-5 (robomaster, case d)


# ---- cameras: project(Xc [n, 3], nudge [n] or None) -> [n, 2], project_jac(Xc) -> [n, 2, 3]
def pinhole_camera(K):
    fx, fy, cx, cy = [float(v) for v in K]

    def project(Xc, nudge=None):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], axis=1)

    def project_jac(Xc):
        x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        J = np.zeros((len(Xc), 2, 3))
        with np.errstate(divide="ignore", invalid="ignore"):
            J[:, 0, 0] = fx / z; J[:, 0, 2] = -fx * x / (z * z)
            J[:, 1, 1] = fy / z; J[:, 1, 2] = -fy * y / (z * z)
        return J
    return project, project_jac


def kb8_camera(p):
    p = np.asarray(p, np.float32)
    return (lambda Xc, nudge=None: ks.project_f64(p, Xc, nudge)), (lambda Xc: ks.project_jac(p, Xc))


# ---- the solve
def _rotations(poses):
    return np.stack([quat_to_R(T[3:]) for T in poses])


def ba_f64(poses, fixed, points, edges, project, project_jac, huber_delta, iterations, active=None, robust=None, nudge=None,
           normalize=True, chi2_prev=None):
    """optimizer.optimize(iterations) on SE3 cameras (t, q_xyzw; fixed or free), XYZ landmarks and one projection edge per record of
    `edges`.  active [E] bool: the edges at level 0 (None: all; a level-1 edge contributes nothing and keeps the chi2 of chi2_prev);
    robust [E] bool: the edges that keep their Huber kernel (None: all, if huber_delta > 0); nudge [E] in {-1, 0, 1}: handed to
    project; normalize: the input quaternions are normalised as SE3Quat's constructor does (False: a further optimize() on the same
    graph).  Returns (poses, points, trials per iteration, stop reason (0 budget, 1 LM terminate, 2 three small steps), edge chi2 at the
    last error evaluation)."""
    poses = np.array(poses, np.float64)
    if normalize:
        poses = np.stack([normalize_pose(T) for T in poses])
    points = np.array(points, np.float64)
    fixed = np.asarray(fixed).astype(bool)
    P, L, E = len(poses), len(points), len(edges)
    ep, el = edges["pose"].astype(np.int64), edges["point"].astype(np.int64)
    obs = np.stack([edges["u"], edges["v"]], axis=1).astype(np.float64)
    info = edges["inv_sigma2"].astype(np.float64)
    act = np.ones(E, bool) if active is None else np.asarray(active).astype(bool)
    rob = (np.ones(E, bool) if robust is None else np.asarray(robust).astype(bool)) & (huber_delta > 0)
    nd = None if nudge is None else np.asarray(nudge)
    d2 = float(huber_delta) * float(huber_delta)
    last = np.zeros(E) if chi2_prev is None else np.array(chi2_prev, np.float64)
    # unknowns: free cameras in vertex order (6 each), then the observed landmarks (3 each)
    used_p = np.zeros(P, bool); used_p[ep] = True
    used_l = np.zeros(L, bool); used_l[el] = True
    free = np.flatnonzero(~fixed & used_p)
    pidx = np.full(P, -1, np.int64); pidx[free] = np.arange(len(free))
    lact = np.flatnonzero(used_l)
    lidx = np.full(L, -1, np.int64); lidx[lact] = np.arange(len(lact))
    n6 = 6 * len(free)
    n = n6 + 3 * len(lact)
    ka = np.flatnonzero(act)
    pfree = pidx[ep[ka]] >= 0
    cols = np.concatenate([np.where(pfree[:, None], 6 * pidx[ep[ka]][:, None] + np.arange(6), 0), n6 + 3 * lidx[el[ka]][:, None] + np.arange(3)], axis=1)

    def residuals(Tp, X):
        R = _rotations(Tp)
        Xc = np.einsum("nij,nj->ni", R[ep[ka]], X[el[ka]]) + Tp[ep[ka], :3]
        e = obs[ka] - project(Xc, None if nd is None else nd[ka])
        c = e[:, 0] * info[ka] * e[:, 0] + e[:, 1] * info[ka] * e[:, 1]
        return R, Xc, e, c

    def errors(Tp, X):
        R, Xc, e, c = residuals(Tp, X)
        last[ka] = c
        with np.errstate(invalid="ignore"):
            r0 = np.where(rob[ka] & (c > d2), 2 * np.sqrt(c) * huber_delta - d2, c)
        return float(np.sum(r0)), R, Xc, e, c

    def system(R, Xc, e, c):
        with np.errstate(invalid="ignore", divide="ignore"):
            r1 = np.where(rob[ka] & (c > d2), huber_delta / np.sqrt(c), 1.0)
        Jp = -project_jac(Xc)
        m = len(ka)
        S = np.zeros((m, 3, 6))
        x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        S[:, 0, 1] = z; S[:, 0, 2] = -y; S[:, 1, 0] = -z; S[:, 1, 2] = x; S[:, 2, 0] = y; S[:, 2, 1] = -x
        S[:, 0, 3] = S[:, 1, 4] = S[:, 2, 5] = 1.0
        J = np.concatenate([np.einsum("nij,njk->nik", Jp, S) * pfree[:, None, None], np.einsum("nij,njk->nik", Jp, R[ep[ka]])], axis=2)   # [m, 2, 9]
        w = r1 * info[ka]
        H = np.zeros((n, n)); b = np.zeros(n)
        np.add.at(H, (cols[:, :, None], cols[:, None, :]), np.einsum("n,nia,nib->nab", w, J, J))
        np.add.at(b, cols, -np.einsum("n,nia,ni->na", w, J, e))
        return H, b

    def apply(Tp, X, x):
        Tn, Xn = Tp.copy(), X.copy()
        for i, p in enumerate(free):
            Tn[p] = oplus(Tp[p], x[6 * i:6 * i + 6])
        Xn[lact] += x[n6:].reshape(-1, 3)
        return Tn, Xn

    lam, ni, nbad, stop = -1.0, 2.0, 0, 0
    trials = []
    x = np.zeros(n)                      # _solver->x(): keeps the last successful solve across a failed one
    for it in range(iterations):
        cur, R, Xc, e, c = errors(poses, points)
        ini = cur
        H, b = system(R, Xc, e, c)
        if it == 0:
            lam, ni, nbad = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0, 0
        qmax, rho = 0, 0.0
        while True:
            ok = True
            try:
                with np.errstate(all="ignore"):
                    cf = scipy.linalg.cho_factor(H + lam * np.eye(n), lower=True, check_finite=True)
                    x = scipy.linalg.cho_solve(cf, b)
            except (np.linalg.LinAlgError, ValueError):
                ok = False
            Tn, Xn = apply(poses, points, x)          # applied and evaluated whether or not the solve succeeded
            temp = errors(Tn, Xn)[0]
            if not ok:
                temp = DMAX
            scale = float(x @ (lam * x + b)) + 1e-3
            rho = (cur - temp) / scale
            if rho > 0 and np.isfinite(temp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha); ni = 2.0; cur = temp
                poses, points = Tn, Xn
            else:
                lam *= ni; ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        trials.append(qmax)
        if qmax == 10 or rho == 0:
            stop = 1
            break
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            stop = 2
            break
    return poses, points, trials, stop, last.copy()


# ---- scenes
def _camera_frame_points(poses, points, edges):
    R = _rotations(poses)
    return np.einsum("nij,nj->ni", R[edges["pose"]], points[edges["point"]]) + poses[edges["pose"], :3]


@functools.lru_cache(maxsize=None)
def ba_scene(model, case, seed):
    """One draw.  model: "robomaster" / "tum" (KannalaBrandt8) or "pinhole" (PINHOLE_K; the same geometry, for the restatement's own check).
    P cameras within a few units of each other, small rotations about a common viewing direction, looking at a cloud 5 to 14 units away; every
    observation at theta in [0.5 deg, 80 deg], 0.7 px of noise, inv_sigma2 = 1.2^(-2 level); every landmark seen at least three times; the
    first n_fixed cameras fixed and exact; free cameras start 0.003 rad / 0.02 off, landmarks 0.03 off; the edge list is in random order
    and holds exactly E edges; gross outliers (+-35 px in u and v) at most one per landmark, only on landmarks with at least six
    observations, on about 30 % of those.  Read-only dict."""
    P, n_fixed, L, E = CASES[case]
    cam = pinhole_camera(PINHOLE_K) if model == "pinhole" else kb8_camera(ks.MODELS[model])
    rng = np.random.default_rng([seed, P, L, E, 18])
    gt = np.zeros((P, 7))
    for p in range(P):
        R = _rot(rng.normal(size=3), rng.uniform(-0.15, 0.15))
        c = rng.uniform(-1.5, 1.5, 3)                          # camera centre
        gt[p] = normalize_pose(np.r_[-R @ c, R_to_quat(R)])
    th = np.deg2rad(40.0) * np.sqrt(rng.uniform(0.0, 1.0, L))
    psi = rng.uniform(-np.pi, np.pi, L)
    d = rng.uniform(5.0, 14.0, L)
    X = np.column_stack([d * np.sin(th) * np.cos(psi), d * np.sin(th) * np.sin(psi), d * np.cos(th)])
    # candidate observations: every (camera, landmark) inside the field
    Rg = _rotations(gt)
    Xc = np.einsum("pij,lj->pli", Rg, X) + gt[:, None, :3]
    theta = np.arctan2(np.hypot(Xc[..., 0], Xc[..., 1]), Xc[..., 2])
    ok = (theta >= THETA_MIN) & (theta <= THETA_MAX)
    must, rest = [], []
    for l in range(L):
        cams = rng.permutation(np.flatnonzero(ok[:, l]))
        if len(cams) < 3:
            raise AssertionError(f"landmark {l} of case {case} seed {seed} is seen by fewer than three cameras")
        must += [(int(p), l) for p in cams[:3]]
        rest += [(int(p), l) for p in cams[3:]]
    if len(must) + len(rest) < E:
        raise AssertionError(f"case {case} seed {seed}: {len(must) + len(rest)} possible observations, {E} wanted")
    pick = rng.permutation(len(rest))[:E - len(must)]
    pairs = np.array(must + [rest[i] for i in pick], np.int64)
    pairs = pairs[rng.permutation(E)]
    edges = np.zeros(E, EDGE_DTYPE)
    edges["pose"], edges["point"] = pairs[:, 0], pairs[:, 1]
    uv = cam[0](Xc[pairs[:, 0], pairs[:, 1]]) + rng.normal(0.0, 1.0, (E, 2)) * 0.7
    n_obs = np.bincount(pairs[:, 1], minlength=L)
    bad = np.zeros(E, bool)
    for l in np.flatnonzero(n_obs >= 6):
        k = rng.choice(np.flatnonzero(pairs[:, 1] == l))
        if rng.random() < 0.3:
            bad[k] = True
    uv[bad] += rng.choice([-1.0, 1.0], size=(int(bad.sum()), 2)) * OUT_SHIFT_PX
    edges["u"], edges["v"] = uv[:, 0], uv[:, 1]
    edges["inv_sigma2"] = 1.2 ** (-2.0 * rng.integers(0, 8, E))
    fixed = np.zeros(P, np.uint8); fixed[:n_fixed] = 1
    poses0 = gt.copy()
    for p in range(n_fixed, P):
        poses0[p] = oplus(gt[p], np.r_[rng.normal(0.0, 0.003, 3), rng.normal(0.0, 0.02, 3)])
    points0 = X + rng.normal(0.0, 0.03, (L, 3))
    nudge = rng.choice([-1, 1], size=E)
    return _freeze(dict(model=model, case=case, seed=seed, p=None if model == "pinhole" else ks.MODELS[model], poses0=poses0, fixed=fixed,
                        points0=np.ascontiguousarray(points0), edges=edges, bad=bad, nudge=nudge, poses_gt=gt, points_gt=X, n_obs=n_obs))


def _camera(model):
    return pinhole_camera(PINHOLE_K) if model == "pinhole" else kb8_camera(ks.MODELS[model])


def _off_axis(poses, points, edges):
    Xc = _camera_frame_points(poses, points, edges)
    return bool(np.all(np.hypot(Xc[:, 0], Xc[:, 1]) >= AXIS_MARGIN * np.abs(Xc[:, 2])))


@functools.lru_cache(maxsize=None)
def ba_ref(model, case, seed):
    """The reference on ba_scene(model, case, seed), as is and with every edge's theta one float32 ulp off, computed once:
    dict(poses, points, trials, stop, chi2; the same with suffix _n; dpose, dpoint, dchi2: the largest differences between the two;
    admissible, why)."""
    sc = ba_scene(model, case, seed)
    pj, jac = _camera(model)
    a = ba_f64(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], pj, jac, HUBER, ITERATIONS)
    b = ba_f64(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], pj, jac, HUBER, ITERATIONS, nudge=sc["nudge"])
    r = dict(poses=a[0], points=a[1], trials=a[2], stop=a[3], chi2=a[4], poses_n=b[0], points_n=b[1], trials_n=b[2], stop_n=b[3], chi2_n=b[4])
    r["dpose"] = float(np.abs(a[0] - b[0]).max()); r["dpoint"] = float(np.abs(a[1] - b[1]).max()); r["dchi2"] = float(np.abs(a[4] - b[4]).max())
    why = []
    if a[2] != b[2] or a[3] != b[3]:
        why.append("the trial sequence moves with one ulp of theta")
    elif float(np.min(np.abs(a[4] - CHI2_MONO))) < BAND_FACTOR * r["dchi2"]:
        why.append("a final chi2 lies within 10 x the chi2 difference of 5.991")
    if not (_off_axis(normalize_all(sc["poses0"]), sc["points0"], sc["edges"]) and _off_axis(a[0], a[1], sc["edges"])):
        why.append("an observation within 1e-3 |z| of the optical axis")
    r["admissible"] = not why; r["why"] = "; ".join(why)
    return _freeze(r)


def normalize_all(poses):
    return np.stack([normalize_pose(T) for T in poses])


def ba_case(model, case):
    """(scene, reference, seed): the first seed in 0 .. MAX_SEEDS - 1 whose draw is admissible.  A case without one fails loudly."""
    why = []
    for seed in range(MAX_SEEDS):
        ref = ba_ref(model, case, seed)
        if ref["admissible"]:
            return ba_scene(model, case, seed), ref, seed
        why.append(f"seed {seed}: {ref['why']}")
    raise AssertionError(f"no admissible scene for {model} case {case}: " + " | ".join(why))


def all_cases():
    return [(m, c) for m in MODELS for c in CASES]


@functools.lru_cache(maxsize=None)
def theta_ulp_ba_diff():
    """The measurement behind THETA_ULP_BA_POSE_DIFF / THETA_ULP_BA_POINT_DIFF on this machine: (largest pose difference, largest point
    difference) between the reference as is and with every edge's theta one float32 ulp off, over the ten admitted scenes."""
    dp = dx = 0.0
    for model, case in all_cases():
        ref = ba_case(model, case)[1]
        dp, dx = max(dp, ref["dpose"]), max(dx, ref["dpoint"])
    return dp, dx


def tolerances():
    """(pose, point) bounds of the GPU test: TOL_FACTOR x the measurement on this machine, TOL_FLOOR at least."""
    dp, dx = theta_ulp_ba_diff()
    return max(TOL_FACTOR * dp, TOL_FLOOR), max(TOL_FACTOR * dx, TOL_FLOOR)


# ---- two rounds on one graph (the welding BA, Optimizer.cc:3474-3519): optimize(5), outliers to level 1 and no robust kernel, optimize(10)
@functools.lru_cache(maxsize=None)
def two_round_ref(model, case, seed):
    """dict(round1 / round2: (poses, points, trials, stop, chi2), flags: [E] uint8 (bit 0 active, bit 1 robust), the same with nudge under
    *_n, dpose, dpoint, dchi2 of round 2, admissible: both rounds' trial sequences and the flags survive the ulp, and no round-1 chi2 lies
    within 10 x its difference of 5.991)."""
    sc = ba_scene(model, case, seed)
    pj, jac = _camera(model)
    out = {}
    for tag, nd in (("", None), ("_n", sc["nudge"])):
        r1 = ba_f64(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], pj, jac, HUBER, 5, nudge=nd)
        active = ~(r1[4] > CHI2_MONO)
        r2 = ba_f64(r1[0], sc["fixed"], r1[1], sc["edges"], pj, jac, HUBER, 10, active=active, robust=np.zeros(len(active), bool), nudge=nd,
                    normalize=False, chi2_prev=r1[4])
        out["round1" + tag], out["round2" + tag], out["flags" + tag] = r1, r2, active.astype(np.uint8)
    a1, a2, b1, b2 = out["round1"], out["round2"], out["round1_n"], out["round2_n"]
    out["dpose"] = float(np.abs(a2[0] - b2[0]).max()); out["dpoint"] = float(np.abs(a2[1] - b2[1]).max())
    out["dchi2_1"] = float(np.abs(a1[4] - b1[4]).max()); out["dchi2"] = float(np.abs(a2[4] - b2[4]).max())
    out["admissible"] = bool(a1[2] == b1[2] and a1[3] == b1[3] and a2[2] == b2[2] and a2[3] == b2[3] and np.array_equal(out["flags"], out["flags_n"])
                             and float(np.min(np.abs(a1[4] - CHI2_MONO))) >= BAND_FACTOR * out["dchi2_1"]
                             and float(np.min(np.abs(a2[4] - CHI2_MONO))) >= BAND_FACTOR * out["dchi2"]
                             and _off_axis(a2[0], a2[1], sc["edges"]))
    return out


def two_round_case(model, case):
    """The first seed whose draw is admissible for the one-round solve AND for the two rounds."""
    for seed in range(MAX_SEEDS):
        if ba_ref(model, case, seed)["admissible"]:
            tr = two_round_ref(model, case, seed)
            if tr["admissible"]:
                return ba_scene(model, case, seed), tr, seed
    raise AssertionError(f"no admissible two-round scene for {model} case {case}")
