"""Scenes for dvm_sim3_hypotheses (Sim3Solver::ComputeSim3 + CheckInliers) and dvm_optimize_sim3 (Optimizer::OptimizeSim3) with two
DIFFERENT cameras, and a float64 restatement of both steps of the solver: horn_f64 (Horn 1987 through numpy.linalg.eigh) and
inliers_f64 (CheckInliers with each camera's own intrinsics and error bounds).  Camera 1's points are laid out at depth ~6 s, so the
pixel geometry of a scene does not depend on its scale.  tests/test_oracle_sim3.py pins the oracle to these on the CPU and pins what
the scenes contain; tests/test_gpu_sim3.py runs the device on them."""
import functools

import numpy as np

K1 = np.array([500.0, 505.0, 320.0, 240.0], np.float32)
K2 = np.array([300.0, 310.0, 310.0, 250.0], np.float32)      # (f1 / f2)^2 = 2.7: exchanging the cameras moves an error well across its bound
ANGLES = (0.0, 1e-4, 0.3, np.pi / 2, 3.0, np.pi - 1e-4, np.pi)
SCALES = (1.0, 0.05, 20.0)
GRID = tuple((a, s) for a in ANGLES for s in SCALES)
GAP_MIN = 1e-3          # hypotheses whose two largest eigenvalues of N lie closer than this (relative) are not compared with float64
BAND = 1e-2             # (hypothesis, point) pairs whose float64 error lies within 1 % of its bound are not compared
GAP_SHARE_MAX = 0.05    # at most this share of a case's hypotheses may be excluded by the gap
BAND_SHARE_MAX = 0.02   # at most this share of a case's pairs may be excluded by the band
SWAP_SHARE_MIN = 0.05   # exchanging the cameras (or the bounds) must change at least this share of the clear pairs

# Largest deviation of the oracle from horn_f64 over the 7 x 3 grid x fix_scale (N = 70, 200 triples, rel_gap > GAP_MIN), measured on
# the CPU (docs/NOTEBOOK.md section 14 lists every case), times 4.  dR: max |R - R64|; ds: |s - s64| / s64; dt: max |t - t64| / (|O1| + s |O2|).
ORACLE_DR_MAX, ORACLE_DS_MAX, ORACLE_DT_MAX = 1.73e-5, 2.91e-7, 1.59e-5
BOUND_DR, BOUND_DS, BOUND_DT = 4 * ORACLE_DR_MAX, 4 * ORACLE_DS_MAX, 4 * ORACLE_DT_MAX
# Near-collinear minimal sets (collinear_scene): the oracle's alignment residual against the float64 optimum, |res - opt| / opt, times 4.
ORACLE_COLLINEAR_RES_MAX = 3.9e-4
BOUND_COLLINEAR_RES = 4 * ORACLE_COLLINEAR_RES_MAX


def rot(axis, angle):
    ax = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def quat_to_R(q):
    """(x, y, z, w), any sign, normalised here."""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _bounds(rng, n):
    """mvnMaxError: (float)(size_t)(9.210 * sigma2) of a random octave."""
    return np.floor(9.210 * (1.2 ** (2 * rng.integers(0, 8, n)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(seed=0, N=70, angle=0.3, scale=1.0, distinct=True, outlier_frac=0.1, noise=0.02):
    """(sc, gt): sc = the keyword arguments of sim3_hypotheses (P1c, P2c float32 [N, 3]; max_err1, max_err2; K1, K2), gt = dict(s, R, t,
    bad).  P1 = s R P2 + t + noise + gross outliers (`noise` is in units of s and grows with the smaller of a point's two bounds, about
    0.3 % of the depth at level 0, so that the errors under a hypothesis from three good points are of the size of the bounds); every depth is positive.  Cached and read-only: the knobs below return changed copies."""
    rng = np.random.default_rng([seed, N, int(distinct)] + [int(x) for x in np.frombuffer(np.float64([angle, scale]).tobytes(), np.uint32)])
    P2 = np.column_stack([rng.uniform(-2, 2, N), rng.uniform(-1.5, 1.5, N), rng.uniform(3, 9, N)])
    R = rot(rng.normal(size=3), angle)
    c2 = np.array([0.0, 0.0, 6.0])
    c1 = scale * np.array([0.3, -0.2, 6.5])           # the cloud turns about its centre and lands in front of camera 1
    t = c1 - scale * (R @ c2)
    e1 = _bounds(rng, N)
    e2 = _bounds(rng, N) if distinct else e1.copy()
    sigma = noise * np.sqrt(np.minimum(e1, e2) / 9.0)            # a keypoint of a coarse level is located less precisely
    P1 = scale * (P2 @ R.T) + t + scale * sigma[:, None] * rng.normal(0, 1.0, (N, 3))
    bad = rng.random(N) < outlier_frac
    P1[bad] += scale * rng.normal(0, 1.0, (int(bad.sum()), 3))
    P1[:, 2] = np.maximum(P1[:, 2], 0.5 * scale)
    sc = dict(P1c=P1.astype(np.float32), P2c=P2.astype(np.float32), max_err1=e1, max_err2=e2, K1=K1.copy(), K2=(K2 if distinct else K1).copy())
    return _freeze(sc), _freeze(dict(s=scale, R=R, t=t, bad=bad))


@functools.lru_cache(maxsize=None)
def triples(seed, N, H):
    """H minimal sets of three distinct indices below N."""
    rng = np.random.default_rng(7919 * seed + 31 * N + H)
    tri = np.array([rng.choice(N, 3, replace=False) for _ in range(H)], np.int32).reshape(H, 3)
    tri.setflags(write=False)
    return tri


@functools.lru_cache(maxsize=None)
def collinear_scene(seed=0, N=70, H=60, off=1e-3, noise=1e-2):
    """(sc, gt, tri): scene(seed, N, 0.3, 1.0) whose first 3 H points are H minimal sets lying within `off` of a line in camera 2 (the two
    largest eigenvalues of N nearly coincide: R is not unique, the alignment residual is), moved to camera 1 with `noise` on each point, so
    that the optimal residual is well above the rounding of the outputs."""
    sc, gt = scene(seed, max(N, 3 * H), 0.3, 1.0)
    rng = np.random.default_rng(seed + 404)
    P1, P2 = sc["P1c"].astype(np.float64), sc["P2c"].astype(np.float64)
    for h in range(H):
        p = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1, 1), rng.uniform(4, 8)])
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        q = np.cross(d, rng.normal(size=3)); q /= np.linalg.norm(q)
        a, b = rng.uniform(0.5, 1.0), rng.uniform(-1.0, -0.5)
        P2[3 * h:3 * h + 3] = [p, p + a * d + rng.uniform(-off, off) * q, p + b * d + rng.uniform(-off, off) * q]
    m = 3 * H
    P1[:m] = gt["s"] * (P2[:m] @ gt["R"].T) + gt["t"] + rng.normal(0, noise, (m, 3))
    tri = np.arange(m, dtype=np.int32).reshape(H, 3)
    tri.setflags(write=False)
    return _freeze(dict(sc, P1c=P1.astype(np.float32), P2c=P2.astype(np.float32))), gt, tri


# ---- knobs: changed copies of a scene dict
def identity(sc):
    """Both cameras see the same coordinates: P1c == P2c bit for bit (the cameras stay as they are)."""
    return dict(sc, P1c=sc["P2c"].copy())


def swap_K(sc):
    return dict(sc, K1=sc["K2"], K2=sc["K1"])


def swap_err(sc):
    return dict(sc, max_err1=sc["max_err2"], max_err2=sc["max_err1"])


def depth0(sc, i):
    """Point i lies in camera 2's principal plane (P2c[i, 2] == 0): FromCameraToImage divides by zero."""
    P2 = sc["P2c"].copy()
    P2[i, 2] = 0.0
    return dict(sc, P2c=P2)


def exact_centroid(sc):
    """The points i whose minimal set [i, i, i] has an exact float centroid in both cameras, ((x + x) + x) / 3 == x for all six coordinates:
    their centred coordinates are exactly 0.  (For the others the centroid is off by an ulp and the solver runs on rounding residue.)"""
    X = np.concatenate([sc["P1c"], sc["P2c"]], axis=1)
    return np.flatnonzero((((X + X) + X) / np.float32(3.0) == X).all(axis=1))


# ---- float64 references
def horn_f64(P1t, P2t, fix_scale=False):
    """Horn's closed form for minimal sets P1t, P2t [H, 3, 3] (set, point, xyz; float32 coordinates taken as exact), all in float64 through
    numpy.linalg.eigh: P1 ~ s R P2 + t with R of the largest eigenvalue of N, s = sum Pr1 . (R Pr2) / sum |R Pr2|^2 as Sim3Solver.cc:358-372
    forms it, t = O1 - s R O2.  Returns (s [H], R [H, 3, 3], t [H, 3], rel_gap [H] = gap of the two largest eigenvalues / largest |eigenvalue|)."""
    P1t = np.asarray(P1t, np.float64).reshape(-1, 3, 3); P2t = np.asarray(P2t, np.float64).reshape(-1, 3, 3)
    O1, O2 = P1t.mean(axis=1), P2t.mean(axis=1)
    A, B = P1t - O1[:, None], P2t - O2[:, None]
    M = np.einsum("hkr,hkc->hrc", B, A)                          # M = Pr2 * Pr1^T
    Nm = np.empty((len(M), 4, 4))
    Nm[:, 0, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    Nm[:, 0, 1] = M[:, 1, 2] - M[:, 2, 1]; Nm[:, 0, 2] = M[:, 2, 0] - M[:, 0, 2]; Nm[:, 0, 3] = M[:, 0, 1] - M[:, 1, 0]
    Nm[:, 1, 1] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]; Nm[:, 1, 2] = M[:, 0, 1] + M[:, 1, 0]; Nm[:, 1, 3] = M[:, 2, 0] + M[:, 0, 2]
    Nm[:, 2, 2] = -M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2]; Nm[:, 2, 3] = M[:, 1, 2] + M[:, 2, 1]
    Nm[:, 3, 3] = -M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]
    for i in range(4):
        for j in range(i):
            Nm[:, i, j] = Nm[:, j, i]
    w, V = np.linalg.eigh(Nm)                                     # ascending
    top = np.abs(w).max(axis=1)
    rel_gap = np.divide(w[:, 3] - w[:, 2], top, out=np.zeros(len(w)), where=top > 0)
    q = V[:, :, 3]
    R = np.stack([quat_to_R([x, y, z, ww]) for ww, x, y, z in q])
    P3 = np.einsum("hrc,hkc->hkr", R, B)
    s = np.ones(len(M)) if fix_scale else np.einsum("hkr,hkr->h", A, P3) / np.einsum("hkr,hkr->h", P3, P3)
    t = O1 - s[:, None] * np.einsum("hrc,hc->hr", R, O2)
    return s, R, t, rel_gap


def align_residual(P1t, P2t, s, R, t):
    """sum over a set's three points of |P1 - (s R P2 + t)|^2, float64, for any (s [H], R [H, 3, 3], t [H, 3])."""
    P1t = np.asarray(P1t, np.float64).reshape(-1, 3, 3); P2t = np.asarray(P2t, np.float64).reshape(-1, 3, 3)
    fit = np.asarray(s, np.float64)[:, None, None] * np.einsum("hrc,hkc->hkr", np.asarray(R, np.float64), P2t) + np.asarray(t, np.float64)[:, None]
    return ((P1t - fit) ** 2).sum(axis=(1, 2))


def unpack(T):
    """T12 [H, 13] -> (s [H], R [H, 3, 3], t [H, 3]) in float64."""
    T = np.asarray(T, np.float64)
    return T[:, 0], T[:, 1:10].reshape(-1, 3, 3), T[:, 10:13]


def deviations(T, sc, tri, fix_scale):
    """(dR, ds, dt, rel_gap), each [H]: T against horn_f64 on the scene's minimal sets, in the units of the bounds above."""
    P1t, P2t = sc["P1c"][tri], sc["P2c"][tri]
    s64, R64, t64, gap = horn_f64(P1t, P2t, fix_scale)
    s, R, t = unpack(T)
    O1 = np.linalg.norm(P1t.astype(np.float64).mean(axis=1), axis=1); O2 = np.linalg.norm(P2t.astype(np.float64).mean(axis=1), axis=1)
    return np.abs(R - R64).max(axis=(1, 2)), np.abs(s - s64) / s64, np.abs(t - t64).max(axis=1) / (O1 + s64 * O2), gap


def inliers_f64(T, sc):
    """CheckInliers in float64 for the similarities T12 [H, 13]: (err1, err2) [H, N], err1 = |proj_K1(P1) - proj_K1(s R P2 + t)|^2 against
    max_err1, err2 = |proj_K2(R^T (P1 - t) / s) - proj_K2(P2)|^2 against max_err2 (Sim3Solver.cc:387-408)."""
    s, R, t = unpack(T)
    P1, P2 = sc["P1c"].astype(np.float64), sc["P2c"].astype(np.float64)
    Ka, Kb = sc["K1"].astype(np.float64), sc["K2"].astype(np.float64)

    def pr(K, X):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.stack([K[0] * X[..., 0] / X[..., 2] + K[2], K[1] * X[..., 1] / X[..., 2] + K[3]], axis=-1)
    X21 = s[:, None, None] * np.einsum("hrc,nc->hnr", R, P2) + t[:, None]
    X12 = np.einsum("hcr,hnc->hnr", R, P1[None] - t[:, None]) / s[:, None, None]
    with np.errstate(invalid="ignore"):
        e1 = ((pr(Ka, P1)[None] - pr(Ka, X21)) ** 2).sum(axis=-1)
        e2 = ((pr(Kb, X12) - pr(Kb, P2)[None]) ** 2).sum(axis=-1)
    return e1, e2


def decide(e1, e2, sc):
    """(inlier [H, N], clear [H, N]): the float64 decision and the pairs whose two errors both lie outside the 1 % band of their bounds."""
    m1, m2 = sc["max_err1"].astype(np.float64), sc["max_err2"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (e1 < m1) & (e2 < m2), (np.abs(e1 - m1) > BAND * m1) & (np.abs(e2 - m2) > BAND * m2)


# ---- OptimizeSim3
def project(K, P):
    return np.c_[K[0] * P[:, 0] / P[:, 2] + K[2], K[1] * P[:, 1] / P[:, 2] + K[3]]


_SIGNS = np.array([[1, 1], [1, -1], [-1, 1], [-1, -1]], np.float64)   # the gross outliers do not pull one way


@functools.lru_cache(maxsize=None)
def sim3_case(seed, N=150, out_frac=0.1, fix_scale=False, noise=0.6, gross=(), s0_scale=None, swap_cameras=False):
    """(S0, P1, P2, obs1, obs2, w1, w2, K1, K2) for optimize_sim3, as _sim3_case of test_gpu_ba.py lays it out, with two different cameras
    (swap_cameras: image 1 is taken with K2 and image 2 with K1).  `gross`: indices whose observation in image 1 is moved by 80 px in u
    and in v (chi2 >= 1000 at any level, against th2 = 10 or 25), the signs cycling so that the outliers do not pull one way: eleven of twenty
    moved by (+80, +80) alike carry the Huber fit with them and nothing survives round 1; `out_frac`: random further outliers at 25 px;
    `noise`: px on every observation.  Read-only (cached).  s0_scale: the scale S0 carries (and, with fix_scale,
    the true one); by default the true scale (drawn from 0.7 .. 1.4, 1 with fix_scale) times 1.05 (times 1 with fix_scale)."""
    from dvm_slam_amd.synth import _quat_from_rot, _rot_from_axis_angle
    rng = np.random.default_rng(seed)
    R = rot(rng.normal(size=3), rng.uniform(-0.4, 0.4))
    t = rng.uniform(-0.5, 0.5, 3)
    s = 1.0 if fix_scale else rng.uniform(0.7, 1.4)
    if fix_scale and s0_scale is not None:
        s = float(s0_scale)
    P2 = np.c_[rng.uniform(-3, 3, N), rng.uniform(-2, 2, N), rng.uniform(4, 12, N)]
    P1 = (s * (R @ P2.T)).T + t
    Ka, Kb = (K2, K1) if swap_cameras else (K1, K2)
    Ka, Kb = Ka.astype(np.float64), Kb.astype(np.float64)
    obs1 = project(Ka, P1) + rng.normal(0, 1.0, (N, 2)) * noise
    obs2 = project(Kb, P2) + rng.normal(0, 1.0, (N, 2)) * noise
    bad = rng.random(N) < out_frac
    obs1[bad] += rng.choice([-1, 1], (int(bad.sum()), 2)) * 25.0
    gross = np.asarray(gross, np.int64)
    obs1[gross] += 80.0 * _SIGNS[np.arange(len(gross)) % 4]
    w1 = 1.2 ** (-2.0 * rng.integers(0, 8, N)); w2 = 1.2 ** (-2.0 * rng.integers(0, 8, N))
    R0 = _rot_from_axis_angle(rng.normal(0, 0.01, 3)) @ R
    s0 = float(s0_scale) if s0_scale is not None else s * (1.0 if fix_scale else 1.05)
    S0 = np.r_[_quat_from_rot(R0), t + rng.normal(0, 0.02, 3), s0]
    out = (S0, P1, P2, obs1, obs2, w1, w2, Ka, Kb)
    for a in out:
        a.setflags(write=False)
    return out


# the OptimizeSim3 cases of tests/test_gpu_sim3.py; tests/test_oracle_sim3.py pins what the oracle returns on each.  survivors: pairs that pass
# round 1 (None: not fixed by construction); second_round: the optimize() length the case is built for (0: early return)
_EVEN = tuple(range(0, 20, 2))
OPT_CASES = {
    "n10": dict(kw=dict(seed=10, N=10, out_frac=0.0), th2=10.0, survivors=10, second_round=5),
    "n255": dict(kw=dict(seed=255, N=255), th2=10.0, survivors=None, second_round=10),
    "n256": dict(kw=dict(seed=256, N=256), th2=10.0, survivors=None, second_round=10),
    "n257": dict(kw=dict(seed=257, N=257), th2=10.0, survivors=None, second_round=10),
    "n513": dict(kw=dict(seed=513, N=513), th2=10.0, survivors=None, second_round=10),
    "n257_swapped": dict(kw=dict(seed=257, N=257, swap_cameras=True), th2=10.0, survivors=None, second_round=10),
    "survive9": dict(kw=dict(seed=40, N=20, out_frac=0.0, noise=0.0, gross=_EVEN + (1,)), th2=10.0, survivors=9, second_round=0),
    "survive10": dict(kw=dict(seed=40, N=20, out_frac=0.0, noise=0.0, gross=_EVEN), th2=10.0, survivors=10, second_round=10),
    "survive11": dict(kw=dict(seed=40, N=20, out_frac=0.0, noise=0.0, gross=_EVEN[:9]), th2=10.0, survivors=11, second_round=10),
    "clean": dict(kw=dict(seed=50, N=60, out_frac=0.0, noise=0.0), th2=10.0, survivors=60, second_round=5),
    "gross3": dict(kw=dict(seed=51, N=60, out_frac=0.0, noise=0.0, gross=(3, 17, 40)), th2=10.0, survivors=57, second_round=10),
    "fix_scale_1.3": dict(kw=dict(seed=52, N=100, fix_scale=True, s0_scale=1.3), th2=10.0, survivors=None, second_round=10),
    "th2_10": dict(kw=dict(seed=53, N=150), th2=10.0, survivors=None, second_round=10),
    "th2_25": dict(kw=dict(seed=53, N=150), th2=25.0, survivors=None, second_round=10),
}


def opt_case(name):
    """(case tuple of sim3_case, fix_scale, th2, spec) of OPT_CASES[name]."""
    spec = OPT_CASES[name]
    return sim3_case(**spec["kw"]), bool(spec["kw"].get("fix_scale", False)), spec["th2"], spec


def chi2_f64(S, P1, P2, obs1, obs2, w1, w2, Ka, Kb):
    """(chi12, chi21) [N] of the two reprojection edges at S = (qx, qy, qz, qw, t, s), float64."""
    R, t, s = quat_to_R(S[:4]), np.asarray(S[4:7], np.float64), float(S[7])
    a = obs1 - project(Ka, s * (P2 @ R.T) + t)
    b = obs2 - project(Kb, ((P1 - t) @ R) / s)
    return w1 * (a ** 2).sum(axis=1), w2 * (b ** 2).sum(axis=1)
