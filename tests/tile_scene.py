"""Linear systems for the tile Cholesky on its own (dvm_tile_solve_debug): tile masks, seeded symmetric positive definite systems whose
condition number is bounded without an eigen-solve, ill-conditioned ones, long double references, and systems whose first non-positive pivot
sits in a chosen row.  Plain numpy, no GPU.

Layout (tile_system.h): unknown block i of `dof` rows lies at tile rows (i // per_tile) * 64 + (i % per_tile) * dof; kept landmark j (3 rows)
at tile ncamt + j // 21, row 3 * (j % 21); x holds block i at dof * i and landmark l at dof * n_blocks + 3 * l."""
import numpy as np
import scipy.linalg

import pg_scene

EPS = pg_scene.EPS
LD = np.longdouble


# ------------------------------------------------------------------------------------------------------------------ layout
def shape(n_blocks, dof=6, per_tile=10, kept_list=(), n_landmarks=0):
    """Rows of a system: tile row and x index of every unknown row, tile counts."""
    kept = np.asarray(kept_list, np.int64)
    ncamt, nkt = -(-n_blocks // per_tile), -(-len(kept) // 21)
    r = np.arange(dof * n_blocks)
    blk = r // dof
    cam_rows = (blk // per_tile) * 64 + (blk % per_tile) * dof + r % dof
    k = np.arange(3 * len(kept))
    kept_rows = (ncamt + k // 63) * 64 + k % 63
    kept_x = dof * n_blocks + 3 * kept[k // 3] + k % 3 if len(kept) else np.zeros(0, np.int64)
    rows = np.concatenate([cam_rows, kept_rows]).astype(np.int64)
    return dict(n_blocks=n_blocks, dof=dof, per_tile=per_tile, kept_list=kept, n_landmarks=n_landmarks, ncamt=ncamt, tiles=ncamt + nkt,
                n=len(rows), rows=rows, tile_of=rows // 64, x_index=np.concatenate([r, kept_x]).astype(np.int64), x_len=dof * n_blocks + 3 * n_landmarks)


# ------------------------------------------------------------------------------------------------------------------ tile masks (lower triangle)
def _mask(t, pairs):
    m = np.eye(t, dtype=np.uint8)
    for i, j in pairs:
        m[max(i, j), min(i, j)] = 1
    return m


def chain_mask(t):
    """t tiles in a path: 1 = single tile, 2 = the pair, 3 and 4 = the pair on top of level launches."""
    return _mask(t, [(i + 1, i) for i in range(t - 1)])


def arrow_mask(k):
    """k leaf columns coupled to one root (tile k) and to nothing else."""
    return _mask(k + 1, [(k, i) for i in range(k)])


def arrow_leaf_counts(schedule, kmax=80):
    """The leaf counts of an arrow on either side of every change of the launcher's path for the leaf level, from the schedule's own strip and
    target counts (schedule: mask -> info dict, capi.tile_schedule_debug).  The launcher's thresholds (tile_launch_cholesky_solve): the level
    in one launch while 4 (ns + nt) <= 256; slices with the diagonal tiles while 4 ns <= 256; solve + update fused while 4 (ns + nt) <= 512.
    Returns {leaf count: expected path name}."""
    def path(k):
        info = schedule(arrow_mask(k))
        ns, nt = info["level_ns"][0], info["level_nt"][0]
        assert info["level_nc"][0] == k and nt > 0
        if 4 * ns <= 256:
            return "level_one_launch" if 4 * (ns + nt) <= 256 else "slices_diag_update"
        return "diag_fused" if 4 * (ns + nt) <= 512 else "diag_trsm_update"
    paths = {k: path(k) for k in range(2, kmax)}
    return {k: p for k, p in paths.items() if paths.get(k - 1, p) != p or paths.get(k + 1, p) != p}


def bush_mask():
    """Two levels of branching: leaves 0 1 -> 2, leaves 3 4 -> 5, 2 and 5 -> root 6."""
    return _mask(7, [(2, 0), (2, 1), (5, 3), (5, 4), (6, 2), (6, 5)])


def two_trees_mask():
    """Two disconnected trees: two roots."""
    return _mask(5, [(1, 0), (2, 1), (4, 3)])


def dense_mask(t):
    return np.tril(np.ones((t, t), np.uint8))


def random_mask(t, seed):
    """A connected random mask: every tile but the last is coupled to a later one, and a few more couplings on top."""
    rng = np.random.default_rng(seed)
    pairs = [(int(rng.integers(i + 1, t)), i) for i in range(t - 1)]
    pairs += [tuple(sorted(rng.choice(t, 2, replace=False), reverse=True)) for _ in range(t // 3)]
    return _mask(t, pairs)


RANDOM_MASKS = tuple((t, seed) for t, seed in ((6, 1), (7, 2), (8, 3), (9, 4), (10, 5), (11, 6), (12, 7), (14, 8)))


def with_kept(cam_mask, kept_tiles, couplings):
    """Kept-landmark tiles behind the camera tiles; couplings: (kept tile index, camera tile) pairs."""
    t = len(cam_mask)
    m = np.eye(t + kept_tiles, dtype=np.uint8)
    m[:t, :t] = cam_mask
    for k, c in couplings:
        m[t + k, c] = 1
    return m


# ------------------------------------------------------------------------------------------------------------------ systems
def dominant_system(mask, sh, seed, empty_tiles=()):
    """Symmetric, non-zero only inside the mask's tiles (tiles listed in empty_tiles stay zero although the mask has them), strictly diagonally
    dominant: the off-diagonal row sum is at most half the diagonal, so by Gershgorin lambda_min >= d_min / 2, lambda_max <= 3 d_max / 2 and
    cond_2 <= 3 d_max / d_min.  Returns dict(A, b, cond) with the full symmetric A."""
    rng = np.random.default_rng(seed)
    n, tile_of = sh["n"], sh["tile_of"]
    assert mask.shape == (sh["tiles"], sh["tiles"])
    allowed = np.array(mask, bool)
    for i, j in empty_tiles:
        allowed[i, j] = False
    allowed |= allowed.T
    A = rng.uniform(-1, 1, (n, n)) * (rng.random((n, n)) < 0.6)
    A = np.tril(A, -1) * allowed[np.ix_(tile_of, tile_of)]
    A = A + A.T
    off = np.abs(A).sum(axis=1)
    d = 2 * np.maximum(off, 1.0) * rng.uniform(1, 3, n)
    A[np.arange(n), np.arange(n)] = d
    return dict(A=A, b=rng.uniform(-1, 1, n) * d, cond=3 * d.max() / d.min(), n=n)


def ill_system(mask, sh, seed, target=1e9):
    """J^T J + lambda I of a graph of relative constraints r = R (x_p - x_q) between blocks, as a bundle adjustment's reduced system looks at
    small lambda: the constant vector is (nearly) in the null space of J, lambda is set so that cond_2 is about `target`.  Only for systems
    without kept landmarks and small enough for an eigen-solve.  Returns dict(A, b, cond) with cond = np.linalg.cond(A)."""
    rng = np.random.default_rng(seed)
    nb, dof, pt = sh["n_blocks"], sh["dof"], sh["per_tile"]
    assert len(sh["kept_list"]) == 0 and sh["n"] <= 900
    edges = [(p + 1, p) for p in range(nb - 1) if (p + 1) // pt == p // pt]
    for i in range(len(mask)):
        for j in range(i):
            if mask[i, j]:
                bi, bj = np.arange(i * pt, min(nb, (i + 1) * pt)), np.arange(j * pt, min(nb, (j + 1) * pt))
                edges += [(int(rng.choice(bi)), int(rng.choice(bj))) for _ in range(3)]
    H = np.zeros((sh["n"], sh["n"]))
    for p, q in edges:
        R = rng.normal(0, 1, (dof, dof))
        G = R.T @ R
        sp, sq = slice(dof * p, dof * p + dof), slice(dof * q, dof * q + dof)
        H[sp, sp] += G; H[sq, sq] += G; H[sp, sq] -= G; H[sq, sp] -= G
    H = (H + H.T) / 2
    A = H + np.linalg.eigvalsh(H)[-1] / target * np.eye(sh["n"])
    return dict(A=A, b=rng.uniform(-1, 1, sh["n"]), cond=float(np.linalg.cond(A)), n=sh["n"])


# ------------------------------------------------------------------------------------------------------------------ references
def solve_refined(A, b):
    """float64 LAPACK Cholesky solve, refined with long double residuals until the correction is below 2^-60 |x|_inf.  Returns longdouble x."""
    F = scipy.linalg.cho_factor(A, lower=True)
    solve = lambda r: scipy.linalg.cho_solve(F, r)
    Al, bl = A.astype(LD), b.astype(LD)
    x = solve(b).astype(LD)
    for _ in range(30):
        dx = solve((bl - Al @ x).astype(np.float64)).astype(LD)
        x = x + dx
        if np.abs(dx).max() <= LD(2.0) ** -60 * np.abs(x).max():
            return x
    raise AssertionError("iterative refinement did not converge")


def solve_ref(A, b):
    """The reference solution: pg_scene.solve_ld (long double Cholesky) up to 700 unknowns, the refined LAPACK solve beyond."""
    return pg_scene.solve_ld(A, b, 0.0) if len(b) <= 700 else solve_refined(A, b)


def solve_f64(A, b):
    """A float64 LAPACK Cholesky solve (potrf + potrs: substitution): the yardstick of the device's residual."""
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), b)


def eta(A, b, x):
    """Normwise backward error |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf) in long double."""
    Al, xl, bl = A.astype(LD), np.asarray(x).astype(LD), b.astype(LD)
    return float(np.abs(bl - Al @ xl).max() / (np.abs(Al).sum(axis=1).max() * np.abs(xl).max() + np.abs(bl).max()))


def forward_bound(sys, x_ref):
    """64 * n * eps * cond * |x_ref|_inf: pg_scene.x_bound's bound with the system's own cond."""
    return 64 * sys["n"] * EPS * sys["cond"] * float(np.abs(x_ref).max())


def expand(sh, x_unknown, x_in):
    """The x the solver leaves: x_in with the unknowns' values at their places."""
    x = np.array(x_in, np.float64, copy=True)
    x[sh["x_index"]] = np.asarray(x_unknown, np.float64)
    return x


# ------------------------------------------------------------------------------------------------------------------ failures
def pivots_ld(A):
    """Pivots d of the long double LDL^T of A, in order, up to and including the first that is not positive."""
    n = len(A)
    Al = A.astype(LD)
    Lm = np.zeros((n, n), LD)
    d = np.zeros(n, LD)
    for r in range(n):
        for c in range(r):
            Lm[r, c] = (Al[r, c] - (Lm[r, :c] * d[:c]) @ Lm[c, :c]) / d[c]
        d[r] = Al[r, r] - (Lm[r, :r] * d[:r]) @ Lm[r, :r]
        if not d[r] > 0:
            return d[:r + 1]
    return d


def break_pivot(A, d, r, kind):
    """A copy of the SPD matrix A (d = pivots_ld(A)) whose pivot r is the first non-positive one: 'negative' (minus half the entry's own size),
    'zero' (only where the pivot IS the entry: nothing before row r couples to it) or 'nan'."""
    B = np.array(A, copy=True)
    if kind == "nan":
        B[r, r] = np.nan
    elif kind == "zero":
        assert not B[r, :r].any()
        B[r, r] = 0.0
    else:
        assert len(d) == len(A) and d[r] > 0      # (pivot r = A[r, r] minus what the rows before it take: only the entry changes)
        B[r, r] = float(LD(A[r, r]) - d[r] - LD(0.5) * LD(A[r, r]))
    return B


def unknown_row(sh, tile, tile_row):
    """The unknown row that lies at `tile_row` of tile `tile` (which must hold an unknown, not padding)."""
    hit = np.flatnonzero(sh["rows"] == 64 * tile + tile_row)
    assert len(hit) == 1
    return int(hit[0])
