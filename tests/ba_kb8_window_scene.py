"""Scenes for the batched local-BA windows on a KannalaBrandt8 camera (dvm_ba_optimize_windows_fast_cam, dvm_ba_pool_optimize_cam):
tests/ba_kb8_scene.py with the SHAPE as an argument.  That file reads its shapes from CASES, which parametrises an existing test and is
not to be touched; the window kernel needs two more:

  w30  (32, 2, 300, 2500)   30 free cameras: the largest reduced system the kernel's LDS holds
  w1   (4, 3, 64, 215)      one free camera (a smaller one, (3, 2, 40, 111), has no admissible seed under tum)

The five shapes a-e of CASES already cover the tails of the eight fixed edge ranges (127, 256 and 257 edges, a ragged last wave) and 21
free cameras; for them this file hands out ba_kb8_scene's own scenes and references (one cache, shared with tests/test_gpu_ba_kb8.py).

  scene(model, shape, seed)   ba_kb8_scene.ba_scene's draw at `shape` = (P, fixed, L, E): the same generator, rng seeded [seed, P, L, E, 18]
  ref(model, shape, seed)     ba_f64 as is and with every edge's theta one float32 ulp off, and ba_kb8_scene.ba_ref's admissibility rule
  case(model, name)           (scene, reference, seed) of the first admissible seed below ba_kb8_scene.MAX_SEEDS
  window_cases()              the 14 (model, name) of the GPU test: robomaster and tum, the seven shapes
  theta_ulp_window_diff()     the tolerance's measurement over exactly those 14 scenes"""
import functools

import numpy as np

import ba_kb8_scene as bs
import kb8_scene as ks
from pose_scene import normalize_pose, oplus, R_to_quat, _rot, _freeze

SHAPES = dict(bs.CASES)
SHAPES["w30"] = (32, 2, 300, 2500)
SHAPES["w1"] = (4, 3, 64, 215)
NEW_SHAPES = ("w30", "w1")
OVER_CAPACITY = (33, 2, 300, 2500)      # 31 free cameras: DVM_ERR_CAPACITY

# Largest differences between ba_f64 as is and with every edge's theta one float32 ulp off, over the 14 admitted scenes of window_cases():
# measured on the CPU (tests/test_ba_kb8_window_scene.py asserts that theta_ulp_window_diff() still lies between half of these and these;
# docs/NOTEBOOK.md section 27 lists the new scenes).  The GPU test allows TOL_FACTOR x the measurement, TOL_FLOOR at least.
THETA_ULP_WIN_POSE_DIFF = 9.5e-7       # measured 9.27e-7 (robomaster, case c: the largest of ba_kb8_scene's ten; w30 / w1 stay below 8.0e-7)
THETA_ULP_WIN_POINT_DIFF = 2.4e-5      # measured 2.3e-5 (tum, w1)


@functools.lru_cache(maxsize=None)
def scene(model, shape, seed):
    """ba_kb8_scene.ba_scene(model, case, seed) with (P, n_fixed, L, E) = shape instead of CASES[case]: statement for statement the same
    draw (tests/test_ba_kb8_window_scene.py holds it to ba_scene bit for bit at shapes a and d).  Read-only dict; `case` is the shape."""
    P, n_fixed, L, E = shape
    cam = bs.pinhole_camera(bs.PINHOLE_K) if model == "pinhole" else bs.kb8_camera(ks.MODELS[model])
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
    Rg = bs._rotations(gt)
    Xc = np.einsum("pij,lj->pli", Rg, X) + gt[:, None, :3]
    theta = np.arctan2(np.hypot(Xc[..., 0], Xc[..., 1]), Xc[..., 2])
    ok = (theta >= bs.THETA_MIN) & (theta <= bs.THETA_MAX)
    must, rest = [], []
    for l in range(L):
        cams = rng.permutation(np.flatnonzero(ok[:, l]))
        if len(cams) < 3:
            raise AssertionError(f"landmark {l} of shape {shape} seed {seed} is seen by fewer than three cameras")
        must += [(int(p), l) for p in cams[:3]]
        rest += [(int(p), l) for p in cams[3:]]
    if len(must) + len(rest) < E:
        raise AssertionError(f"shape {shape} seed {seed}: {len(must) + len(rest)} possible observations, {E} wanted")
    pick = rng.permutation(len(rest))[:E - len(must)]
    pairs = np.array(must + [rest[i] for i in pick], np.int64)
    pairs = pairs[rng.permutation(E)]
    edges = np.zeros(E, bs.EDGE_DTYPE)
    edges["pose"], edges["point"] = pairs[:, 0], pairs[:, 1]
    uv = cam[0](Xc[pairs[:, 0], pairs[:, 1]]) + rng.normal(0.0, 1.0, (E, 2)) * 0.7
    n_obs = np.bincount(pairs[:, 1], minlength=L)
    bad = np.zeros(E, bool)
    for l in np.flatnonzero(n_obs >= 6):
        k = rng.choice(np.flatnonzero(pairs[:, 1] == l))
        if rng.random() < 0.3:
            bad[k] = True
    uv[bad] += rng.choice([-1.0, 1.0], size=(int(bad.sum()), 2)) * bs.OUT_SHIFT_PX
    edges["u"], edges["v"] = uv[:, 0], uv[:, 1]
    edges["inv_sigma2"] = 1.2 ** (-2.0 * rng.integers(0, 8, E))
    fixed = np.zeros(P, np.uint8); fixed[:n_fixed] = 1
    poses0 = gt.copy()
    for p in range(n_fixed, P):
        poses0[p] = oplus(gt[p], np.r_[rng.normal(0.0, 0.003, 3), rng.normal(0.0, 0.02, 3)])
    points0 = X + rng.normal(0.0, 0.03, (L, 3))
    nudge = rng.choice([-1, 1], size=E)
    return _freeze(dict(model=model, case=tuple(shape), seed=seed, p=None if model == "pinhole" else ks.MODELS[model], poses0=poses0, fixed=fixed,
                        points0=np.ascontiguousarray(points0), edges=edges, bad=bad, nudge=nudge, poses_gt=gt, points_gt=X, n_obs=n_obs))


@functools.lru_cache(maxsize=None)
def ref(model, shape, seed):
    """ba_kb8_scene.ba_ref on scene(model, shape, seed): the same two solves, the same differences, the same admissibility rule."""
    sc = scene(model, shape, seed)
    pj, jac = bs._camera(model)
    a = bs.ba_f64(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], pj, jac, bs.HUBER, bs.ITERATIONS)
    b = bs.ba_f64(sc["poses0"], sc["fixed"], sc["points0"], sc["edges"], pj, jac, bs.HUBER, bs.ITERATIONS, nudge=sc["nudge"])
    r = dict(poses=a[0], points=a[1], trials=a[2], stop=a[3], chi2=a[4], poses_n=b[0], points_n=b[1], trials_n=b[2], stop_n=b[3], chi2_n=b[4])
    r["dpose"] = float(np.abs(a[0] - b[0]).max()); r["dpoint"] = float(np.abs(a[1] - b[1]).max()); r["dchi2"] = float(np.abs(a[4] - b[4]).max())
    why = []
    if a[2] != b[2] or a[3] != b[3]:
        why.append("the trial sequence moves with one ulp of theta")
    elif float(np.min(np.abs(a[4] - bs.CHI2_MONO))) < bs.BAND_FACTOR * r["dchi2"]:
        why.append("a final chi2 lies within 10 x the chi2 difference of 5.991")
    if not (bs._off_axis(bs.normalize_all(sc["poses0"]), sc["points0"], sc["edges"]) and bs._off_axis(a[0], a[1], sc["edges"])):
        why.append("an observation within 1e-3 |z| of the optical axis")
    r["admissible"] = not why; r["why"] = "; ".join(why)
    return _freeze(r)


def case(model, name):
    """(scene, reference, seed) of the first admissible seed.  Shapes a-e: ba_kb8_scene.ba_case itself.  A shape without one fails loudly."""
    if name in bs.CASES:
        return bs.ba_case(model, name)
    why = []
    for seed in range(bs.MAX_SEEDS):
        r = ref(model, SHAPES[name], seed)
        if r["admissible"]:
            return scene(model, SHAPES[name], seed), r, seed
        why.append(f"seed {seed}: {r['why']}")
    raise AssertionError(f"no admissible scene for {model} shape {name}: " + " | ".join(why))


def pinhole_twin(name, seed):
    """The pinhole scene of the same shape and seed (ba_kb8_scene.PINHOLE_K)."""
    return bs.ba_scene("pinhole", name, seed) if name in bs.CASES else scene("pinhole", SHAPES[name], seed)


def window_cases():
    return [(m, n) for n in SHAPES for m in bs.MODELS]      # robomaster and tum alternate


@functools.lru_cache(maxsize=None)
def theta_ulp_window_diff():
    """The measurement behind THETA_ULP_WIN_POSE_DIFF / THETA_ULP_WIN_POINT_DIFF on this machine, over the 14 admitted scenes."""
    dp = dx = 0.0
    for model, name in window_cases():
        r = case(model, name)[1]
        dp, dx = max(dp, r["dpose"]), max(dx, r["dpoint"])
    return dp, dx


def tolerances():
    """(pose, point) bounds of the GPU test: TOL_FACTOR x the measurement on this machine, TOL_FLOOR at least."""
    dp, dx = theta_ulp_window_diff()
    return max(bs.TOL_FACTOR * dp, bs.TOL_FLOOR), max(bs.TOL_FACTOR * dx, bs.TOL_FLOOR)
