"""orc_pose_graph_trial (one iteration body of the oracle's essential-graph optimiser, stage by stage) pinned on the CPU: e and J against
mpmath at 50 digits -- J against the SAME central differences (delta = 1e-9), i.e. g2o's specification without rounding -- and H, b, x, the
update and the sums against the stage bounds that tests/test_gpu_pose_graph.py then asks of the device (tests/pg_scene.py)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import pg_scene as pgs  # noqa: E402

EPS = pgs.EPS
LAMBDAS = (1e-16, 1.0)
ALL = pgs.FAMILY_NAMES


def _mp_ctx():
    import mpmath

    class Ctx:
        mp = mpmath.mp
        sqrt, sin, cos, exp, log, atan2 = mpmath.sqrt, mpmath.sin, mpmath.cos, mpmath.exp, mpmath.log, mpmath.atan2
        small = 0          # the exact limits only where an argument IS zero

        @staticmethod
        def num(v):
            return mpmath.mpf(float(v))
    mpmath.mp.dps = 50
    return Ctx


_trials = {}


def trial(oracle, name, fix, lam):
    key = (name, fix, lam)
    if key not in _trials:
        sc = pgs.family(name)
        _trials[key] = oracle.pose_graph_trial(sc["S"], sc["fixed"], sc["edges_v"], sc["edges_meas"], fix_scale=fix, lam=lam)
    return _trials[key]


def test_scenes_contain_what_they_claim():
    """The paths the graphs exist for are in them: fixed vertices on both sides, an edge between fixed vertices, both orientations of a
    pair, a duplicate, an untouched free vertex, two components, every tile boundary."""
    assert sorted(int((sc["fixed"] == 0).sum()) for sc in pgs.families()[:len(pgs.CHAIN_SIZES)]) == sorted(pgs.CHAIN_SIZES)
    fa = pgs.family("fixed_anywhere14")
    fx, ev = fa["fixed"], fa["edges_v"]
    assert not fx[0] and fx[7] and fx[13] and fx.sum() == 2
    for f in (7, 13):
        assert (fx[ev[:, 0]] & (ev[:, 0] == f) & ~fx[ev[:, 1]].astype(bool)).any() and (fx[ev[:, 1]] & (ev[:, 1] == f) & ~fx[ev[:, 0]].astype(bool)).any()
    assert (fx[ev[:, 0]] & fx[ev[:, 1]]).sum() == 1
    mo = pgs.family("mixed_orientation11")
    pairs = [tuple(p) for p in mo["edges_v"].tolist()]
    assert all((j, i) in pairs for (i, j) in pairs) and len(pairs) - len(set(pairs)) == 1
    k = pairs.index((1, 0))
    assert np.allclose(pgs.sim3_mul(list(mo["edges_meas"][k]), list(mo["edges_meas"][pairs.index((0, 1))])), [0, 0, 0, 1, 0, 0, 0, 1], atol=1e-15)
    iso = pgs.family("isolated10")
    assert not iso["fixed"][4] and 4 not in iso["edges_v"]
    st = pgs.family("star40")
    assert (st["edges_v"] == 1).any(axis=1).sum() == 41 and (st["edges_v"][:, 0] == 1).sum() > 10 and (st["edges_v"][:, 1] == 1).sum() > 10
    tc = pgs.family("two_components16")
    assert tc["fixed"][[0, 10]].all() and tc["fixed"].sum() == 2 and not ((tc["edges_v"][:, 0] < 8) ^ (tc["edges_v"][:, 1] < 8)).any()
    assert pgs.family("two_components16_floating")["fixed"].sum() == 1
    assert len(pgs.family("clique12")["edges_v"]) == 66
    for sc in pgs.families():
        assert np.array_equal(pgs.normalise(sc["S"]), sc["S"]) or np.abs(pgs.normalise(sc["S"]) - sc["S"]).max() <= EPS


def test_pins_e_and_J(oracle):
    """e and J of the oracle against mpmath (50 digits): E_DEV and J_DEV of pg_scene.py are the maxima printed here.  With fix_scale the
    first six columns of J are the same numbers bit for bit and column 6 is exactly zero; a fixed vertex's side is exactly zero."""
    ctx = _mp_ctx()
    e_dev = j_dev = 0.0
    for name in ALL:
        sc = pgs.family(name)
        o = trial(oracle, name, False, 1.0)
        e_mp = pgs.errors(ctx, sc)
        de = max(abs(float(e_mp[k][a] - ctx.num(o["e"][k, a]))) for k in range(len(e_mp)) for a in range(7))
        dj = 0.0
        for k in range(len(e_mp)):
            J = pgs.jacobian(ctx, sc, k)
            dj = max(dj, max(abs(float(J[s][a][d] - ctx.num(o["J"][k, s, a, d]))) for s in range(2) for a in range(7) for d in range(7)))
        print(f"{name}: |e - mp| = {de:.3e}  |J - mp| = {dj:.3e}")
        e_dev, j_dev = max(e_dev, de), max(j_dev, dj)
        assert np.abs(pgs.error_f64(sc) - o["e"]).max() <= 2 * pgs.BOUND_E        # the float64 reference sits within the same distance
        of = trial(oracle, name, True, 1.0)
        assert np.array_equal(of["e"], o["e"]) and np.array_equal(of["J"][..., :6], o["J"][..., :6]) and not of["J"][..., 6].any()
        for s in range(2):
            assert not o["J"][sc["fixed"][sc["edges_v"][:, s]] != 0, s].any()
    print(f"E_DEV = {e_dev:.3e}  J_DEV = {j_dev:.3e}")
    assert e_dev <= pgs.E_DEV and j_dev <= pgs.J_DEV
    assert pgs.E_DEV <= 2 * e_dev and pgs.J_DEV <= 2 * j_dev      # the recorded constants are the measured ones, not a generous guess


def test_jacobian_reference_is_a_derivative():
    """The central differences in mpmath agree with a much finer difference quotient (delta^2 truncation only): the reference measures
    rounding, not its own step."""
    ctx = _mp_ctx()
    sc = pgs.family("ring12")
    J = pgs.jacobian(ctx, sc, 3)
    old = pgs.DELTA
    try:
        pgs.DELTA = 1e-20
        Jf = pgs.jacobian(ctx, sc, 3)
    finally:
        pgs.DELTA = old
    assert max(abs(float(J[s][a][d] - Jf[s][a][d])) for s in range(2) for a in range(7) for d in range(7)) < 1e-15


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_oracle_stages(oracle, name, fix, lam):
    """The oracle's H, b, x, update and sums meet the stage bounds the device is asked to meet."""
    pgs.check_stages(trial(oracle, name, fix, lam), pgs.family(name), fix, lam, f"oracle {name} fix={int(fix)} lam={lam:g}")


def test_oracle_trial_is_the_optimisers_first_trial(oracle):
    """One iteration of orc_pose_graph_optimize = orc_pose_graph_trial at lambda 1e-16 when that trial is accepted: same estimates, same
    chi2, bit for bit (they share the body)."""
    sc = pgs.family("ring12")
    t = trial(oracle, "ring12", False, 1e-16)
    S, st = oracle.pose_graph_optimize(sc["S"], sc["fixed"], sc["edges_v"], sc["edges_meas"], iterations=1)
    assert st[38] == 1 and st[2] == t["chi2_before"] and st[3] == t["chi2_after"] and np.array_equal(S, t["S"])


def test_oracle_failure_flag(oracle):
    """lambda = -1 on the clique: the factorisation meets a non-positive pivot, x stays zero, the estimates stay; lambda = 1 on a
    component without a fixed vertex is an ordinary solve."""
    sc = pgs.family("clique12")
    t = oracle.pose_graph_trial(sc["S"], sc["fixed"], sc["edges_v"], sc["edges_meas"], lam=-1.0)
    assert t["failed"] == 1 and not t["x"].any() and np.array_equal(t["S"], sc["S"])
    fl = pgs.family("two_components16_floating")
    pgs.check_stages(oracle.pose_graph_trial(fl["S"], fl["fixed"], fl["edges_v"], fl["edges_meas"], lam=1.0), fl, False, 1.0, "oracle floating lam=1")
