"""GPU parity of the two Sim3 kernels on two DIFFERENT cameras (tests/sim3_scene.py; tests/test_oracle_sim3.py pins the scenes and the
oracle on the CPU): dvm_sim3_hypotheses (k_sim3_hypotheses: Sim3Solver::ComputeSim3 + CheckInliers, one wave per hypothesis) and
dvm_optimize_sim3 (k_optimize_sim3: Optimizer::OptimizeSim3, one workgroup).

Bounds of the hypothesis tests.  Device and oracle share jacobi4 operation for operation (-ffp-contract=off on both sides); only atan2 / sin /
cos can differ, in the last double bit, before R is cast to float.  So R agrees to one float ulp of a value <= 1, 2^-23; s = nom / den over sums
through R to 1e-6 relative; t = O1 - s R O2 (nine float terms) to 1e-6 (|O1| + s |O2|).  None of them is tuned to what the device gives."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import sim3_scene as ss  # noqa: E402

pytestmark = pytest.mark.gpu

N, H = 70, 200
ULP = 2.0 ** -23
I13 = np.r_[1.0, np.eye(3).ravel(), 0.0, 0.0, 0.0].astype(np.float32)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _both(capi, oracle, sc, tri, fix, key=None):
    """((Tg, ng, mg), (To, no, mo)); with a key the pair is computed once for all the tests that look at it."""
    if key is not None and key in _cache:
        return _cache[key]
    out = capi.sim3_hypotheses(triples=tri, fix_scale=fix, **sc), oracle.sim3_hypotheses(triples=tri, fix_scale=fix, **sc)
    if key is not None:
        _cache[key] = out
    return out


def _grid(capi, oracle, angle, scale, fix):
    sc, gt = ss.scene(0, N, angle, scale)
    tri = ss.triples(0, N, H)
    return (sc, tri) + _both(capi, oracle, sc, tri, fix, ("grid", angle, scale, fix))


def _assert_tight(dev, orc, sc, tri):
    """The 1-ulp bounds on T, count == mask sum, and the masks: bit-equal rows of T give bit-equal mask rows; elsewhere a differing pair
    lies inside the 1 % band of the float64 errors under the oracle's T.  Returns the bit-equal rows."""
    (Tg, ng, mg), (To, no, mo) = dev, orc
    assert Tg.shape == To.shape and mg.shape == mo.shape
    sg, Rg, tg = ss.unpack(Tg); so, Ro, to = ss.unpack(To)
    P1t, P2t = sc["P1c"][tri].astype(np.float64), sc["P2c"][tri].astype(np.float64)
    tnorm = np.linalg.norm(P1t.mean(axis=1), axis=1) + np.abs(so) * np.linalg.norm(P2t.mean(axis=1), axis=1)
    dR, ds, dt = np.abs(Rg - Ro).max(), (np.abs(sg - so) / np.abs(so)).max(), (np.abs(tg - to).max(axis=1) / tnorm).max()
    print(f"dR {dR:.3e} ds {ds:.3e} dt {dt:.3e}")
    assert dR <= ULP and ds <= 1e-6 and dt <= 1e-6
    assert np.array_equal(ng, mg.sum(axis=1)) and set(np.unique(mg)) <= {0, 1}
    eq = (_bits(Tg) == _bits(To)).all(axis=1)
    assert np.array_equal(mg[eq], mo[eq]) and np.array_equal(ng[eq], no[eq])
    if (~eq).any():
        ref, clear = ss.decide(*ss.inliers_f64(To[~eq], sc), sc)
        assert not ((mg[~eq] != mo[~eq]) & clear).any()
    return eq


# ---- dvm_sim3_hypotheses
@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("angle,scale", ss.GRID)
def test_grid_parity(capi, oracle, angle, scale, fix):
    """Rotation angle {0, 1e-4, 0.3, pi/2, 3.0, pi - 1e-4, pi} x scale {1, 0.05, 20} x fix_scale against the oracle, tight; at least half of
    a case's rows of T are bit-equal, so the mask comparison is not empty."""
    sc, tri, dev, orc = _grid(capi, oracle, angle, scale, fix)
    eq = _assert_tight(dev, orc, sc, tri)
    print(f"rows of T not bit-equal: {(~eq).sum()} of {H}")
    assert eq.mean() >= 0.5


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("angle,scale", ss.GRID)
def test_grid_against_float64(capi, oracle, angle, scale, fix):
    """The device against horn_f64 / inliers_f64 directly, with the CPU test's exclusions and caps: its deviation is at most twice the
    oracle's largest on the same case + 1e-6, its decisions equal the float64 ones on the clear pairs."""
    sc, tri, (Tg, ng, mg), (To, no, mo) = _grid(capi, oracle, angle, scale, fix)
    assert np.isfinite(Tg).all()
    dg, do = ss.deviations(Tg, sc, tri, fix), ss.deviations(To, sc, tri, fix)
    ok = dg[3] > ss.GAP_MIN
    assert (~ok).mean() <= ss.GAP_SHARE_MAX
    for k, name in enumerate(("R", "s", "t")):
        print(f"{name}: device {dg[k][ok].max():.3e} oracle {do[k][ok].max():.3e}")
        assert dg[k][ok].max() <= 2 * do[k][ok].max() + 1e-6
    ref, clear = ss.decide(*ss.inliers_f64(Tg, sc), sc)
    assert (~clear).mean() <= ss.BAND_SHARE_MAX
    assert np.array_equal(mg.astype(bool)[clear], ref[clear])


@pytest.mark.parametrize("fix", [False, True])
def test_collinear_sets(capi, fix):
    """Three points within 1e-3 of a line: R is not unique, the alignment residual is; against the float64 optimum."""
    sc, gt, tri = ss.collinear_scene()
    P1t, P2t = sc["P1c"][tri], sc["P2c"][tri]
    s64, R64, t64, gap = ss.horn_f64(P1t, P2t, fix)
    opt = ss.align_residual(P1t, P2t, s64, R64, t64)
    T, nin, mask = capi.sim3_hypotheses(triples=tri, fix_scale=fix, **sc)
    assert np.isfinite(T).all() and np.array_equal(nin, mask.sum(axis=1))
    rel = np.abs(ss.align_residual(P1t, P2t, *ss.unpack(T)) - opt) / opt
    print(f"residual excess {rel.max():.3e}")
    assert rel.max() <= ss.BOUND_COLLINEAR_RES


def test_identity_rows(capi, oracle):
    """P1c == P2c: vn == 0, the guarded division: R == I, s == 1, t == 0 exactly, the oracle's bits, every point an inlier."""
    for seed, n in ((0, 70), (1, 129)):
        sc = ss.identity(ss.scene(seed, n, 0.0, 1.0)[0])
        tri = ss.triples(seed, n, H)
        for fix in (False, True):
            (Tg, ng, mg), (To, no, mo) = _both(capi, oracle, sc, tri, fix)
            assert np.array_equal(_bits(Tg), _bits(To)) and np.array_equal(Tg, np.broadcast_to(I13, Tg.shape))
            assert (ng == n).all() and mg.all()


def test_repeated_index_rows(capi, oracle):
    """One launch mixes good minimal sets with [i, i, i] (NaN rows, see test_oracle_sim3.test_repeated_index_rows) and [i, i, j] / [j, i, i]
    (two distinct points): those rows equal the oracle's, NaN for NaN; the NaN rows have no inlier; the good rows of the launch have the bits
    of a launch without the bad ones."""
    sc, gt = ss.scene(0, N, 0.3, 1.0)
    ex = ss.exact_centroid(sc)
    j = [int(np.setdiff1d(np.flatnonzero(~gt["bad"]), [i])[k]) for k, i in enumerate(ex)]
    bad_rows = np.array([[i, i, i] for i in ex] + [[i, i, jj] for i, jj in zip(ex, j)] + [[jj, i, i] for i, jj in zip(ex, j)], np.int32)
    good = ss.triples(0, N, 100)
    tri = np.concatenate([good, bad_rows])
    order = np.random.default_rng(3).permutation(len(tri))
    tri = tri[order]
    is_bad = order >= len(good)
    is_nan = is_bad & (order < len(good) + len(ex))
    (Tg, ng, mg), (To, no, mo) = _both(capi, oracle, sc, tri, False)
    assert np.isnan(To[is_nan][:, [0, 10, 11, 12]]).all() and np.isfinite(To[~is_nan]).all()
    assert np.array_equal(Tg[is_bad], To[is_bad], equal_nan=True)
    assert np.array_equal(Tg[is_nan][:, 1:10], np.broadcast_to(I13[1:10], (int(is_nan.sum()), 9)))
    assert not mg[is_nan].any() and not ng[is_nan].any()
    assert np.array_equal(mg[is_bad], mo[is_bad]) and np.array_equal(ng[is_bad], no[is_bad])
    T0, n0, m0 = capi.sim3_hypotheses(triples=good, fix_scale=False, **sc)
    back = np.argsort(order)[:len(good)]                       # where the good rows went
    assert np.array_equal(_bits(Tg[back]), _bits(T0)) and np.array_equal(mg[back], m0) and np.array_equal(ng[back], n0)
    _assert_tight((Tg[back], ng[back], mg[back]), (To[back], no[back], mo[back]), sc, good)


def test_depth_zero_point(capi, oracle):
    sc, gt = ss.scene(0, N, 0.3, 1.0)
    tri = ss.triples(0, N, H)
    i = int(np.argmax(oracle.sim3_hypotheses(triples=tri, fix_scale=False, **sc)[2].sum(axis=0)))
    tri = tri[~(tri == i).any(axis=1)]
    d = ss.depth0(sc, i)
    dev, orc = _both(capi, oracle, d, tri, False)
    assert not dev[2][:, i].any()
    _assert_tight(dev, orc, d, tri)
    T0, n0, m0 = capi.sim3_hypotheses(triples=tri, fix_scale=False, **sc)
    assert m0[:, i].mean() > 0.3
    assert np.array_equal(_bits(T0), _bits(dev[0])) and np.array_equal(np.delete(m0, i, axis=1), np.delete(dev[2], i, axis=1))


def _guarded_call(capi, sc, tri, fix):
    """dvm_sim3_hypotheses on buffers one row longer than the launch needs, the outputs pre-filled: (T, nin, mask) in full."""
    L = capi.lib()
    vp, i32 = C.c_void_p, C.c_int32
    L.dvm_sim3_hypotheses.restype = i32
    L.dvm_sim3_hypotheses.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp]
    a = [np.ascontiguousarray(sc[k], np.float32) for k in ("P1c", "P2c", "max_err1", "max_err2", "K1", "K2")]
    tr = np.ascontiguousarray(tri, np.int32)
    n, h = len(a[0]), len(tr)
    T = np.full((h + 1, 13), 7.5, np.float32); nin = np.full(h + 1, -77, np.int32); mask = np.full((h + 1, n), 0xAA, np.uint8)
    p = lambda x: x.ctypes.data_as(vp)
    capi.check(L.dvm_sim3_hypotheses(0, p(a[0]), p(a[1]), p(a[2]), p(a[3]), n, p(a[4]), p(a[5]), p(tr), h, int(fix), p(T), p(nin), p(mask)))
    return T, nin, mask


@pytest.mark.parametrize("n,h,angle,scale", [(3, 50, 0.3, 1.0), (63, 50, 0.3, 1.0), (64, 50, 3.0, 20.0), (65, 50, 0.3, 1.0), (127, 50, np.pi, 0.05),
                                             (128, 50, 0.3, 1.0), (129, 50, 0.3, 1.0), (1000, 50, 3.0, 0.05),
                                             (129, 1, 0.3, 1.0), (129, 2, 0.3, 1.0), (129, 1000, 0.3, 1.0), (1000, 1000, 0.3, 1.0)])
def test_sizes(capi, oracle, n, h, angle, scale):
    """The ballot loop's full wave, one over and one under, N = 3, H = 1, and the largest launch: the whole [H, N] mask against the oracle's
    (a lane past N that wrote would land in row h + 1), and one more row of every output buffer untouched."""
    sc, gt = ss.scene(2, n, angle, scale)
    tri = ss.triples(2, n, h)
    orc = oracle.sim3_hypotheses(triples=tri, fix_scale=False, **sc)
    T, nin, mask = _guarded_call(capi, sc, tri, False)
    assert (T[h] == 7.5).all() and nin[h] == -77 and (mask[h] == 0xAA).all()
    _assert_tight((T[:h], nin[:h], mask[:h]), orc, sc, tri)
    if h >= 50:
        assert orc[1].max() >= (2 if n == 3 else 0.3 * n)       # the scene is solvable at this size


def test_rows_are_independent(capi):
    """The same 300 minimal sets as one launch, permuted, ten of them alone, and the launch again: a row's bits depend on its set only."""
    sc, gt = ss.scene(0, 129, 0.3, 1.0)
    tri = ss.triples(5, 129, 300)
    T, nin, mask = capi.sim3_hypotheses(triples=tri, fix_scale=False, **sc)
    T2, nin2, mask2 = capi.sim3_hypotheses(triples=tri, fix_scale=False, **sc)
    assert np.array_equal(_bits(T), _bits(T2)) and np.array_equal(nin, nin2) and np.array_equal(mask, mask2)
    perm = np.random.default_rng(9).permutation(300)
    Tp, ninp, maskp = capi.sim3_hypotheses(triples=tri[perm], fix_scale=False, **sc)
    assert np.array_equal(_bits(Tp), _bits(T[perm])) and np.array_equal(ninp, nin[perm]) and np.array_equal(maskp, mask[perm])
    for r in np.random.default_rng(10).choice(300, 10, replace=False):
        T1, nin1, mask1 = capi.sim3_hypotheses(triples=tri[r:r + 1], fix_scale=False, **sc)
        assert np.array_equal(_bits(T1[0]), _bits(T[r])) and nin1[0] == nin[r] and np.array_equal(mask1[0], mask[r])


@pytest.mark.parametrize("knob", [ss.swap_K, ss.swap_err], ids=["K1<->K2", "max_err1<->max_err2"])
@pytest.mark.parametrize("angle,scale", [(0.3, 1.0), (3.0, 20.0), (np.pi, 0.05)])
def test_swap_sensitivity(capi, oracle, angle, scale, knob):
    """The device called with the cameras (or the bounds) exchanged agrees with the oracle called the same way, and decides at least 5 % of
    the pairs that are clear in both calls differently from the unswapped call: the scene tells camera 1 from camera 2."""
    sc, tri, (Tg, ng, mg), (To, no, mo) = _grid(capi, oracle, angle, scale, False)
    sw = knob(sc)
    dev, orc = _both(capi, oracle, sw, tri, False)
    _assert_tight(dev, orc, sw, tri)
    assert np.array_equal(_bits(dev[0]), _bits(Tg))             # the similarity does not depend on either
    clear = ss.decide(*ss.inliers_f64(To, sc), sc)[1] & ss.decide(*ss.inliers_f64(To, sw), sw)[1]
    share = (dev[2] != mg)[clear].mean()
    print(f"decided differently: {share:.3f}")
    assert share >= ss.SWAP_SHARE_MIN


# ---- dvm_optimize_sim3
@pytest.mark.parametrize("name", list(ss.OPT_CASES))
def test_optimize_sim3(capi, oracle, name):
    """Sim3 within 1e-6 of the oracle, identical inlier mask and count, on two different cameras: the 256-thread stride tails, the survivor
    boundary 9 / 10 / 11, both lengths of the second round, fix_scale at 1.3, th2 10 and 25 (test_oracle_sim3 pins each case)."""
    (S0, *rest), fix, th2, spec = ss.opt_case(name)
    So, io, no = oracle.optimize_sim3(S0, fix, *rest, th2)
    Sg, ig, ng = capi.optimize_sim3(S0, fix, *rest, th2)
    assert ng == no and np.array_equal(ig, io)
    if spec["second_round"] == 0:
        assert ng == 0 and not ig.any() and np.array_equal(_bits(Sg), _bits(np.asarray(S0)))
        return
    assert ng >= 10 and ng == ig.sum()
    print(f"|S - S_oracle| {np.abs(Sg - So).max():.3e}")
    assert np.abs(Sg - So).max() < 1e-6
    if spec["survivors"] is not None:
        assert ng == spec["survivors"]
    if fix:
        assert np.array_equal(_bits(Sg[7:8]), _bits(np.float64([1.3])))


def test_optimize_sim3_quaternion_sign(capi, oracle):
    """S0 given as q and as -q: the same similarity."""
    (S0, *rest), fix, th2, _ = ss.opt_case("n257")
    Sa, ia, na = capi.optimize_sim3(S0, fix, *rest, th2)
    Sb, ib, nb = capi.optimize_sim3(np.r_[-S0[:4], S0[4:]], fix, *rest, th2)
    assert na == nb and np.array_equal(ia, ib)
    assert np.abs(ss.quat_to_R(Sa[:4]) - ss.quat_to_R(Sb[:4])).max() < 1e-12 and np.abs(Sa[4:] - Sb[4:]).max() < 1e-12
    So, io, no = oracle.optimize_sim3(np.r_[-S0[:4], S0[4:]], fix, *rest, th2)
    assert nb == no and np.array_equal(ib, io) and np.abs(Sb - So).max() < 1e-6
