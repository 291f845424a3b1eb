"""Pose graphs for the stage-by-stage tests of the essential-graph optimiser, and plain references of every stage.

Graphs (each builder takes a size and a seed; poses are drawn as in synth.pose_graph: keyframes on a loop, drift 0.02 accumulated into the
initial estimates, measurements Sji = Sjw * Swi from the ground truth with noise 0.003): chain, ring, star, clique, two_components,
mixed_orientation, fixed_anywhere, isolated.  `families()` lists the cases the tests run, `relabel` permutes vertex ids and edge order.

References: sim3 algebra written once over a small "context" (math for float64, mpmath for tests/test_oracle_pose_graph.py -- this file
never imports mpmath), error_f64, jacobian (the central differences g2o takes, delta = 1e-9, in whatever arithmetic the context has),
assemble (H and b from GIVEN J and e with math.fsum, plus the sum of absolute values and the number of terms of every entry),
solve_ld (np.longdouble Cholesky), update_f64.

tests/test_oracle_pose_graph.py pins the oracle to these on the CPU; tests/test_gpu_pose_graph.py runs the device on them."""
import functools
import math

import numpy as np

EPS = 2.0 ** -52
DRIFT, NOISE = 0.02, 0.003
DELTA = 1e-9                      # g2o's numeric differentiation step (base_binary_edge.hpp)

# Largest deviation of the oracle's e and J (orc_pose_graph_trial) from the same quantities evaluated with mpmath at 50 digits, over
# families() with fix_scale = 0 (J with fix_scale = 1 is the same numbers with column 6 zero), measured on the CPU by
#   python -m pytest tests/test_oracle_pose_graph.py -k "pins_e_and_J" -s
# e is a few ulp of values below 1; J divides rounding of that size by 2e-9.
E_DEV = 9.1e-15
J_DEV = 6.1e-6
BOUND_E, BOUND_J = 4 * E_DEV, 4 * J_DEV


# ------------------------------------------------------------------------------------------------- Sim3 algebra over a context
class FloatCtx:
    """float64 through the math module, with g2o's own case distinctions (sim3.h:128-197, eps = 1e-5): below them A, B, C take g2o's
    values and Sim3::log takes omega = deltaR / 2.  g2o's B for a small angle and a scale that is not small,
    ((sigma^2 / 2 - sigma + 1) s) / sigma^3, is NOT the limit of the general formula (that one ends in `s - 1`): it is what the
    reference computes, the oracle and the device follow it, and so does this context.  It matters only once the errors are small, i.e.
    for chi2 after a step; the linearisation points of the scenes lie outside these branches (E_DEV would show it)."""
    sqrt, sin, cos, exp, log, atan2 = math.sqrt, math.sin, math.cos, math.exp, math.log, math.atan2
    small = 1e-5
    g2o = True

    @staticmethod
    def num(v):
        return float(v)


F64 = FloatCtx


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _qmul(a, b):   # Hamilton product, (x, y, z, w)
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz]


def _qrot(q, v):   # R(q) v = v + 2 w (u x v) + 2 u x (u x v)
    u, w = q[:3], q[3]
    c1 = _cross(u, v)
    c2 = _cross(u, c1)
    return [v[i] + 2 * (w * c1[i] + c2[i]) for i in range(3)]


def _abc(ctx, theta, sigma, s):
    """A, B, C of W = A Omega + B Omega^2 + C I = integral of exp(tau (sigma I + Omega)) over [0, 1] (the exact limits below `small`)."""
    ts, ss = abs(theta) <= ctx.small, abs(sigma) <= ctx.small
    if ss:
        C = ctx.num(1)
        if ts:
            return ctx.num(1) / 2, ctx.num(1) / 6, C
        return (1 - ctx.cos(theta)) / (theta * theta), (theta - ctx.sin(theta)) / (theta * theta * theta), C
    C = (s - 1) / sigma
    if ts:
        s2 = sigma * sigma
        return ((sigma - 1) * s + 1) / s2, ((s2 / 2 - sigma + 1) * s - (0 if getattr(ctx, "g2o", False) else 1)) / (s2 * sigma), C
    a, b, c = s * ctx.sin(theta), s * ctx.cos(theta), theta * theta + sigma * sigma
    return (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) / (theta * theta), C


def _W(A, B, C, om):
    O = [[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]]
    O2 = [[sum(O[i][k] * O[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
    return [[A * O[i][j] + B * O2[i][j] + (C if i == j else 0) for j in range(3)] for i in range(3)]


def sim3_exp(ctx, u):
    """g2o::Sim3(update): u = (omega, upsilon, sigma) -> (q_xyzw, t, s) as a list of 8."""
    om, up, sigma = list(u[:3]), list(u[3:6]), u[6]
    theta = ctx.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2])
    s = ctx.exp(sigma)
    if theta == 0:
        q = [ctx.num(0), ctx.num(0), ctx.num(0), ctx.num(1)]
    else:
        k = ctx.sin(theta / 2) / theta
        q = [k * om[0], k * om[1], k * om[2], ctx.cos(theta / 2)]
    A, B, C = _abc(ctx, theta, sigma, s)
    W = _W(A, B, C, om)
    t = [sum(W[i][j] * up[j] for j in range(3)) for i in range(3)]
    return q + t + [s]


def sim3_mul(a, b):
    rt = _qrot(a[:4], b[4:7])
    return _qmul(a[:4], b[:4]) + [a[7] * rt[i] + a[4 + i] for i in range(3)] + [a[7] * b[7]]


def sim3_inv(a):
    q = [-a[0], -a[1], -a[2], a[3]]
    rt = _qrot(q, [-a[4] / a[7], -a[5] / a[7], -a[6] / a[7]])
    return q + rt + [1 / a[7]]


def sim3_log(ctx, S):
    """g2o Sim3::log: (omega, upsilon, sigma) with upsilon = W^-1 t."""
    q, t, s = S[:4], S[4:7], S[7]
    sigma = ctx.log(s)
    qn = ctx.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    v, w = [q[i] / qn for i in range(3)], q[3] / qn
    if w < 0:
        v, w = [-c for c in v], -w
    vn = ctx.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if vn == 0:
        theta, om = ctx.num(0), [ctx.num(0)] * 3
    else:
        theta = 2 * ctx.atan2(vn, w)
        om = [theta * c / vn for c in v]
    if getattr(ctx, "g2o", False) and 1 - 2 * vn * vn > 1 - ctx.small:       # d = cos(theta) > 1 - eps: omega = deltaR / 2 = sin(theta) axis
        om = [2 * w * c for c in v]
        theta = ctx.num(0)
    A, B, C = _abc(ctx, theta, sigma, s)
    W = _W(A, B, C, om)
    c00, c01, c02 = W[1][1] * W[2][2] - W[1][2] * W[2][1], W[1][2] * W[2][0] - W[1][0] * W[2][2], W[1][0] * W[2][1] - W[1][1] * W[2][0]
    det = W[0][0] * c00 + W[0][1] * c01 + W[0][2] * c02
    inv = [[c00, W[0][2] * W[2][1] - W[0][1] * W[2][2], W[0][1] * W[1][2] - W[0][2] * W[1][1]],
           [c01, W[0][0] * W[2][2] - W[0][2] * W[2][0], W[0][2] * W[1][0] - W[0][0] * W[1][2]],
           [c02, W[0][1] * W[2][0] - W[0][0] * W[2][1], W[0][0] * W[1][1] - W[0][1] * W[1][0]]]
    return om + [(inv[i][0] * t[0] + inv[i][1] * t[1] + inv[i][2] * t[2]) / det for i in range(3)] + [sigma]


def edge_error(ctx, C, Si, Sj):
    """EdgeSim3::computeError: log(C * Si * Sj^-1)."""
    return sim3_log(ctx, sim3_mul(sim3_mul(C, Si), sim3_inv(Sj)))


def _lift(ctx, row):
    return [ctx.num(v) for v in row]


def errors(ctx, sc):
    """e[E][7] of a scene in the context's arithmetic (lists of context numbers)."""
    S = [_lift(ctx, r) for r in sc["S"]]
    return [edge_error(ctx, _lift(ctx, m), S[i], S[j]) for (i, j), m in zip(sc["edges_v"], sc["edges_meas"])]


def error_f64(sc):
    return np.array(errors(F64, sc), np.float64)


def jacobian(ctx, sc, k, fix_scale=False):
    """J[2][7][7] ([side][error row][dof]) of edge k: central differences with delta = 1e-9 on oplus (S <- Sim3(u) * S), evaluated in the
    context's arithmetic -- with mpmath this is g2o's specification without rounding.  A fixed vertex's side is zero."""
    i, j = sc["edges_v"][k]
    C, X = _lift(ctx, sc["edges_meas"][k]), [_lift(ctx, sc["S"][i]), _lift(ctx, sc["S"][j])]
    d1 = ctx.num(DELTA)
    J = [[[ctx.num(0)] * 7 for _ in range(7)] for _ in range(2)]
    for side in range(2):
        if sc["fixed"][(i, j)[side]]:
            continue
        for d in range(7):
            ev = []
            for sgn in (1, -1):
                u = [ctx.num(0)] * 7
                u[d] = sgn * d1
                if fix_scale:
                    u[6] = ctx.num(0)
                Y = list(X)
                Y[side] = sim3_mul(sim3_exp(ctx, u), X[side])
                ev.append(edge_error(ctx, C, Y[0], Y[1]))
            for a in range(7):
                J[side][a][d] = (ev[0][a] - ev[1][a]) / (2 * d1)
    return J


# ------------------------------------------------------------------------------------------------------------ the graphs
def normalise(S):
    """Unit quaternions as dvm_pose_graph_optimize makes them on entry (same operations, same order)."""
    S = np.array(S, np.float64, copy=True)
    q = S[:, :4]
    nn = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    S[:, :4] = q / nn[:, None]
    return S


def _small(rng, sd_rot, sd_t, sd_s):
    return sim3_exp(F64, list(rng.normal(0, sd_rot, 3)) + list(rng.normal(0, sd_t, 3)) + [rng.normal(0, sd_s)])


def _poses(n, rng):
    """Ground truth on a loop and the drifted initial estimates, as synth.pose_graph draws them."""
    gt = []
    for i in range(n):
        a = 2 * math.pi * i / max(n, 3)
        yaw, pitch, roll = a + math.pi / 2, 0.1 * math.sin(3 * a), 0.05 * math.cos(2 * a)
        qz = [0, 0, math.sin(yaw / 2), math.cos(yaw / 2)]
        qy = [0, math.sin(pitch / 2), 0, math.cos(pitch / 2)]
        qx = [math.sin(roll / 2), 0, 0, math.cos(roll / 2)]
        Twc = _qmul(_qmul(qz, qy), qx) + [10 * math.cos(a), 10 * math.sin(a), 0.3 * math.sin(4 * a), 1.0]
        gt.append(sim3_inv(Twc))
    S0, acc = [list(gt[0])], [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for i in range(1, n):
        acc = sim3_mul(_small(rng, DRIFT, 5 * DRIFT, DRIFT), acc)
        S0.append(sim3_mul(acc, gt[i]))
    return gt, S0


def _scene(name, n, pairs, fixed, seed, inverse_of=None, duplicate_of=None):
    """pairs: (i, j) per edge.  inverse_of[k] = m: edge k carries the inverse of edge m's measurement (k runs the other way);
    duplicate_of[k] = m: an exact copy."""
    rng = np.random.default_rng(seed)
    gt, S0 = _poses(n, rng)
    meas = []
    for k, (i, j) in enumerate(pairs):
        if inverse_of and k in inverse_of:
            meas.append(sim3_inv(meas[inverse_of[k]]))
        elif duplicate_of and k in duplicate_of:
            meas.append(list(meas[duplicate_of[k]]))
        else:
            meas.append(sim3_mul(_small(rng, NOISE, NOISE, NOISE), sim3_mul(gt[j], sim3_inv(gt[i]))))
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    sc = dict(name=name, S0=np.array(S0, np.float64), fixed=fx, edges_v=np.array(pairs, np.int32).reshape(-1, 2),
              edges_meas=np.array(meas, np.float64).reshape(-1, 8))
    sc["S"] = normalise(sc["S0"])    # what both sides linearise at
    for v in sc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc


@functools.lru_cache(maxsize=None)
def chain(nfree, seed=1):
    return _scene(f"chain{nfree}", nfree + 1, [(i, i - 1) for i in range(1, nfree + 1)], [0], seed)


@functools.lru_cache(maxsize=None)
def ring(n=12, seed=2):
    return _scene(f"ring{n}", n, [(i, i - 1) for i in range(1, n)] + [(n - 1, 0)], [0], seed)


@functools.lru_cache(maxsize=None)
def star(spokes=40, seed=3):
    """Vertex 0 fixed, vertex 1 the hub: its diagonal block collects spokes + 1 contributions, alternately as vertex i and vertex j."""
    pairs = [(1, 0)] + [((1, v) if v % 2 else (v, 1)) for v in range(2, spokes + 2)]
    return _scene(f"star{spokes}", spokes + 2, pairs, [0], seed)


@functools.lru_cache(maxsize=None)
def clique(n=12, seed=4):
    return _scene(f"clique{n}", n, [(i, j) for i in range(n) for j in range(i)], [0], seed)


@functools.lru_cache(maxsize=None)
def two_components(n=16, seed=5, fix_second=True):
    """Vertices [0, h) and [h, n): two rings without an edge between them.  The first is held at vertex 0, the second at h + 2 (or
    nowhere: a floating component, solvable only through the damping)."""
    h = n // 2
    pairs = [(i, i - 1) for i in range(1, h)] + [(h - 1, 0)] + [(i, i - 1) for i in range(h + 1, n)] + [(n - 1, h)]
    return _scene(f"two_components{n}" + ("" if fix_second else "_floating"), n, pairs, [0, h + 2] if fix_second else [0], seed)


@functools.lru_cache(maxsize=None)
def mixed_orientation(n=11, seed=6):
    """A ring with a chord per vertex; every pair carries (i, j) and (j, i), the second with the inverse measurement, plus one exact
    duplicate: every off-diagonal block collects contributions of both orientations."""
    base = [(i, i - 1) for i in range(1, n)] + [(n - 1, 0)] + [(i, i - 3) for i in range(3, n)]
    pairs, inverse_of = [], {}
    for (i, j) in base:
        pairs.append((i, j))
        pairs.append((j, i))
        inverse_of[len(pairs) - 1] = len(pairs) - 2
    pairs.append(pairs[4])
    return _scene(f"mixed_orientation{n}", n, pairs, [0], seed, inverse_of=inverse_of, duplicate_of={len(pairs) - 1: 4})


@functools.lru_cache(maxsize=None)
def fixed_anywhere(n=14, seed=7):
    """Fixed = {n // 2, n - 1}; vertex 0 is free.  Both fixed vertices are vertex i of some edges and vertex j of others, and one edge
    joins the two."""
    m = n // 2
    pairs = [(i, i - 1) for i in range(1, n)] + [(0, n - 1), (m + 2, m), (m, m - 2), (2, n - 1), (n - 1, m)]
    return _scene(f"fixed_anywhere{n}", n, pairs, [m, n - 1], seed)


@functools.lru_cache(maxsize=None)
def isolated(n=10, seed=8):
    """A chain of n vertices and one more free vertex, in the middle of the ids, that no edge touches."""
    ids = [v for v in range(n + 1) if v != 4]
    return _scene(f"isolated{n}", n + 1, [(ids[i], ids[i - 1]) for i in range(1, n)], [0], seed)


CHAIN_SIZES = (1, 2, 8, 9, 10, 18, 19, 28)     # free vertices: one, two and three-plus tile columns of 9, both sides of each boundary


@functools.lru_cache(maxsize=None)
def families():
    return tuple([chain(k) for k in CHAIN_SIZES] + [ring(), star(), clique(), two_components(), mixed_orientation(), fixed_anywhere(), isolated()])


def family(name):
    return {sc["name"]: sc for sc in families() + (two_components(fix_second=False),)}[name]


FAMILY_NAMES = tuple(sc["name"] for sc in families())


def relabel(sc, seed=99):
    """The same graph with vertex ids and edge order permuted.  Returns (scene, perm, eperm): new vertex id of old vertex v = perm[v],
    new edge number m holds old edge eperm[m]."""
    rng = np.random.default_rng(seed)
    n, E = len(sc["S0"]), len(sc["edges_v"])
    perm, eperm = rng.permutation(n), rng.permutation(E)
    out = dict(name=sc["name"] + "_relabelled")
    for key in ("S0", "S", "fixed"):
        a = np.empty_like(sc[key])
        a[perm] = sc[key]
        out[key] = a
    out["edges_v"] = perm[sc["edges_v"][eperm]].astype(np.int32)
    out["edges_meas"] = sc["edges_meas"][eperm].copy()
    return out, perm, eperm


def free_ids(sc):
    return np.flatnonzero(np.asarray(sc["fixed"]) == 0)


# --------------------------------------------------------------------------------------------------------- stage references
def assemble(J, e, sc):
    """H = J^T J (lower triangle, NO damping) and b = -J^T e in vertex-id order of the free vertices from GIVEN J[E,2,7,7] and e[E,7]:
    every entry is math.fsum of its terms J_a[k][r] * J_b[k][c] (resp. J[k][r] * -e[k]).  Returns dict(H, b, Habs, babs, Hn, bn,
    structure): abs = sum of |terms|, n = number of terms (0 outside the structure), structure = boolean mask of the entries that
    have a block."""
    ids = free_ids(sc)
    num = {int(v): a for a, v in enumerate(ids)}
    dim = 7 * len(ids)
    hterms, bterms = {}, {}
    for k, (vi, vj) in enumerate(np.asarray(sc["edges_v"]).tolist()):
        for sa, va in enumerate((vi, vj)):
            if va not in num:
                continue
            bterms.setdefault(num[va], []).append(J[k, sa] * (-e[k])[:, None])            # [error row, r]
            for sb, vb in enumerate((vi, vj)):
                if vb in num and num[va] >= num[vb]:
                    hterms.setdefault((num[va], num[vb]), []).append(J[k, sa][:, :, None] * J[k, sb][:, None, :])   # [error row, r, c]
    out = dict(H=np.zeros((dim, dim)), Habs=np.zeros((dim, dim)), Hn=np.zeros((dim, dim), np.int64), b=np.zeros(dim), babs=np.zeros(dim),
               bn=np.zeros(dim, np.int64), structure=np.zeros((dim, dim), bool))
    for a in range(len(ids)):
        out["structure"][7 * a:7 * a + 7, 7 * a:7 * a + 7] = np.tril(np.ones((7, 7), bool))     # every free vertex owns its diagonal block
    for (a, c), tl in hterms.items():
        t = np.concatenate(tl, axis=0)
        for r in range(7):
            for q in range(r + 1 if a == c else 7):
                col = t[:, r, q]
                out["H"][7 * a + r, 7 * c + q] = math.fsum(col)
                out["Habs"][7 * a + r, 7 * c + q] = math.fsum(np.abs(col))
                out["Hn"][7 * a + r, 7 * c + q] = len(col)
                out["structure"][7 * a + r, 7 * c + q] = True
    for a, tl in bterms.items():
        t = np.concatenate(tl, axis=0)
        for r in range(7):
            out["b"][7 * a + r] = math.fsum(t[:, r])
            out["babs"][7 * a + r] = math.fsum(np.abs(t[:, r]))
            out["bn"][7 * a + r] = len(t)
    return out


def symmetric(L):
    """Full symmetric matrix of a lower triangle."""
    return np.tril(L) + np.tril(L, -1).T


def solve_ld(H, b, lam):
    """(H + lam I) x = b by Cholesky in np.longdouble (H: full symmetric float64).  Returns x as longdouble."""
    n = len(b)
    A = np.array(H, np.longdouble) + np.longdouble(lam) * np.eye(n, dtype=np.longdouble)
    L = np.zeros((n, n), np.longdouble)
    for r in range(n):
        for c in range(r):
            L[r, c] = (A[r, c] - L[r, :c] @ L[c, :c]) / L[c, c]
        d = A[r, r] - L[r, :r] @ L[r, :r]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[r, r] = np.sqrt(d)
    y = np.zeros(n, np.longdouble)
    for r in range(n):
        y[r] = (np.longdouble(b[r]) - L[r, :r] @ y[:r]) / L[r, r]
    x = np.zeros(n, np.longdouble)
    for r in range(n - 1, -1, -1):
        x[r] = (y[r] - L[r + 1:, r] @ x[r + 1:]) / L[r, r]
    return x


def h_bound(ref, lam):
    """(n_terms + 2) * eps * sum |terms| for every entry of H.  On the diagonal lambda is added last: it enters the sum of magnitudes and
    is not counted as a term (the oracle's worst entry sits at 0.21 of this bound, 0.17 off the diagonal, 0.10 for b)."""
    return (ref["Hn"] + 2) * EPS * (ref["Habs"] + abs(lam) * np.eye(len(ref["b"])))


def x_bound(H_ref, lam, x_ref):
    """Forward bound of the solve: 64 * dim * eps * cond2(H_ref + lam I) * |x_ref|_inf."""
    n = len(x_ref)
    cond = np.linalg.cond(np.asarray(H_ref, np.float64) + lam * np.eye(n))
    return 64 * n * EPS * cond * float(np.abs(x_ref).max()), cond


def update_f64(S, x, fixed, fix_scale):
    """oplus in float64: S_v <- Sim3(x_v) * S_v for the free vertices (x in vertex-id order), scale frozen by fix_scale."""
    out = np.array(S, np.float64, copy=True)
    for a, v in enumerate(np.flatnonzero(np.asarray(fixed) == 0)):
        u = [float(c) for c in x[7 * a:7 * a + 7]]
        if fix_scale:
            u[6] = 0.0
        out[v] = sim3_mul(sim3_exp(F64, u), [float(c) for c in S[v]])
    return out


def update_scale(S):
    """What 'per component' is measured against in the update check: 1 for the unit quaternion, the largest |t| of the vertex (at least 1)
    for the translation -- t' = s R t + t_x sums terms of that size -- and s for the scale."""
    S = np.asarray(S)
    sc = np.ones_like(S)
    sc[:, 4:7] = np.maximum(1.0, np.abs(S[:, 4:7]).max(axis=1))[:, None]
    sc[:, 7] = np.abs(S[:, 7])
    return sc


def check_stages(t, sc, fix, lam, tag, S_lin=None):
    """The stage bounds of one trial `t` (oracle's or device's dict) against the references, from ITS OWN e and J.  Used by tests/test_oracle_pose_graph.py (the oracle
    meets them on the CPU) and tests/test_gpu_pose_graph.py (the device).  Returns the measured x error as a fraction of its bound."""
    E, ids = len(sc["edges_v"]), free_ids(sc)
    S_lin = sc["S"] if S_lin is None else S_lin      # the estimates the trial linearised at (the device normalises its input once more)
    nfree, dim = len(ids), 7 * len(ids)
    e, J = t["e"], t["J"]
    # chi2 = sum e^2: 7E products, recursive or tree summation
    chi_ref = math.fsum((e * e).ravel())
    assert abs(t["chi2_before"] - chi_ref) <= 7 * E * EPS * chi_ref, (tag, t["chi2_before"], chi_ref)
    # H and b from the trial's own J and e
    ref = assemble(J, e, sc)
    Hl = np.tril(t["H"])
    assert not Hl[~ref["structure"]].any(), (tag, "entries outside the structure")
    Href = ref["H"] + lam * np.eye(dim)
    bad = np.argwhere(np.abs(Hl - Href) > h_bound(ref, lam))
    assert not len(bad), (tag, "H", bad[:4].tolist(), [(Hl[r, c], Href[r, c]) for r, c in bad[:4]], t.get("vidx"))
    lone = ref["Habs"].diagonal() == 0        # diagonal entries without a non-zero term: exactly lambda (isolated vertex; column 6 with fix_scale)
    assert np.array_equal(Hl.diagonal()[lone], np.full(int(lone.sum()), lam)), tag
    if fix:
        assert lone[6::7].all() and not Hl[6::7, :][:, np.arange(dim) % 7 != 6].any() and not Hl[:, 6::7][np.arange(dim) % 7 != 6, :].any(), tag
    bbad = np.flatnonzero(np.abs(t["b"] - ref["b"]) > (ref["bn"] + 2) * EPS * ref["babs"])
    assert not len(bbad), (tag, "b", bbad[:4].tolist(), t.get("vidx"))
    if sc["name"].startswith("isolated"):
        a = int(np.searchsorted(ids, 4))
        blk = Hl[7 * a:7 * a + 7]
        assert np.array_equal(blk[:, 7 * a:7 * a + 7], lam * np.eye(7)) and not np.delete(blk, np.s_[7 * a:7 * a + 7], axis=1).any(), tag
        assert not Hl[:, 7 * a:7 * a + 7][np.r_[0:7 * a, 7 * a + 7:dim]].any() and not t["b"][7 * a:7 * a + 7].any(), tag
    # x against the long double solve of the reference system
    Hs = symmetric(ref["H"])
    # rows whose diagonal entry has no non-zero term (column 6 under fix_scale, the vertex without edges) hold lambda alone: H is exactly
    # zero beside them and b is exactly zero (both asserted above), so their x is exactly 0 and the rest of the system stands on its own.
    # With them left in, cond2 is about 1e18 at lambda = 1e-16 and the bound says nothing; the bound is taken on the system without them.
    keep = ~lone
    assert not t["b"][lone].any() and not t["x"][lone].any(), (tag, "x of a lambda-only row")
    Hk = Hs[np.ix_(keep, keep)]
    x_ref = solve_ld(Hk, ref["b"][keep], lam)
    xb, cond = x_bound(Hk, lam, x_ref.astype(np.float64))
    xerr = float(np.abs(t["x"][keep] - x_ref).max())
    ratio = xerr / xb if xb > 0 else 0.0
    print(f"{tag}: cond = {cond:.2e}  |x - x_ref| = {xerr:.2e}  bound = {xb:.2e}  ratio = {ratio:.2e}")
    assert not t["failed"] and xerr <= xb, (tag, xerr, xb)
    # update from the trial's own x
    S_ref = update_f64(S_lin, t["x"], sc["fixed"], fix)
    assert (np.abs(t["S"] - S_ref) <= 16 * EPS * update_scale(S_ref)).all(), (tag, "update", np.abs((t["S"] - S_ref) / update_scale(S_ref)).max() / EPS)
    fx = sc["fixed"] != 0
    assert np.array_equal(t["S"][fx], S_lin[fx]), (tag, "a fixed vertex moved")
    if fix:
        assert np.array_equal(t["S"][:, 7], S_lin[:, 7]), (tag, "scale moved under fix_scale")
    # computeScale = x^T (lambda x + b) from the trial's own x and b: 2 * 7 nfree products
    terms = np.concatenate([lam * t["x"] * t["x"], t["x"] * t["b"]])
    assert abs(t["scale_sum"] - math.fsum(terms)) <= 14 * nfree * EPS * math.fsum(np.abs(terms)), (tag, "computeScale")
    # chi2 after: the errors at the new estimates (float64 reference; its own rounding is a few ulp of each e)
    after = dict(sc)
    after["S"] = t["S"]
    e_after = error_f64(after)
    chi_after, de = math.fsum((e_after ** 2).ravel()), 12 * E_DEV     # 4 E_DEV device - oracle, 8 E_DEV oracle - error_f64 (pinned on the CPU)
    assert abs(t["chi2_after"] - chi_after) <= de * (2 * np.abs(e_after).sum() + 7 * E * de) + 7 * E * EPS * chi_after, (tag, t["chi2_after"], chi_after)
    return ratio
