"""The essential-graph optimiser stage by stage: ONE trial of dvm_pose_graph_optimize (dvm_pose_graph_debug_trial: same set-up, same
launches) against plain references on the graphs of tests/pg_scene.py -- fixed vertices anywhere and on either side of an edge, an edge
between fixed vertices, both orientations of a pair and a duplicate, a free vertex without edges, two components, 1 to 28 free vertices
(every boundary of the 9-vertex tiles).

e and J are compared with the oracle (4 x its own distance from mpmath, pinned by tests/test_oracle_pose_graph.py); everything behind
them is a deterministic function of the device's OWN e and J and is held to bounds derived from the arithmetic: H and b entry by entry
against math.fsum, x against a long double Cholesky, the update, computeScale and chi2.  The public entry point then runs the same graphs
for 20 iterations."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import pg_scene as pgs  # noqa: E402

pytestmark = pytest.mark.gpu
LAMBDAS = (1e-16, 1.0)
ALL = pgs.FAMILY_NAMES
_cache = {}


def _args(sc):
    return sc["S"], sc["fixed"], sc["edges_v"], sc["edges_meas"]


def dev_trial(capi, sc, fix, lam):
    key = ("dev", sc["name"], fix, lam)
    if key not in _cache:
        _cache[key] = capi.pose_graph_debug_trial(*_args(sc), fix_scale=fix, lam=lam)
    return _cache[key]


def orc_trial(oracle, sc, fix, lam):
    key = ("orc", sc["name"], fix, lam)
    if key not in _cache:
        _cache[key] = oracle.pose_graph_trial(*_args(sc), fix_scale=fix, lam=lam)
    return _cache[key]


def reference(t, sc):
    key = ("ref", sc["name"], id(t))
    if key not in _cache:
        _cache[key] = pgs.assemble(t["J"], t["e"], sc)
    return _cache[key]


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_trial_stages(capi, oracle, name, fix, lam):
    """e and J against the oracle (4 E_DEV, 4 J_DEV; exact zeros for a fixed vertex's side and for column 6 under fix_scale), then chi2,
    H, b, x, the updated estimates, computeScale and chi2 after the trial from the device's own e and J (pg_scene.check_stages)."""
    sc = pgs.family(name)
    g, o = dev_trial(capi, sc, fix, lam), orc_trial(oracle, sc, fix, lam)
    de, dj = np.abs(g["e"] - o["e"]).max(), np.abs(g["J"] - o["J"]).max()
    print(f"{name} fix={int(fix)} lam={lam:g}: |e - oracle| = {de:.2e} (bound {pgs.BOUND_E:.2e})  |J - oracle| = {dj:.2e} (bound {pgs.BOUND_J:.2e})")
    assert de <= pgs.BOUND_E and dj <= pgs.BOUND_J
    for side in range(2):
        assert not g["J"][sc["fixed"][sc["edges_v"][:, side]] != 0, side].any(), "J of a fixed vertex"
        assert g["J"][sc["fixed"][sc["edges_v"][:, side]] == 0, side].any(axis=(1, 2)).all(), "J of a free vertex"
    if fix:
        assert not g["J"][..., 6].any()
    assert np.array_equal(g["vidx"] < 0, sc["fixed"] != 0) and sorted(g["vidx"][g["vidx"] >= 0]) == list(range(g["nfree"]))
    pgs.check_stages(g, sc, fix, lam, f"device {name} fix={int(fix)} lam={lam:g}", S_lin=pgs.normalise(sc["S"]))


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", ALL)
def test_trial_relabelled(capi, name, lam):
    """Vertex ids and edge order permuted: e and J are the same numbers edge by edge, the relabelled trial meets the stage bounds on its
    own structure, and H, b (assembly bound) and x (x bound) mapped back agree with the original labelling's."""
    sc = pgs.family(name)
    rl, perm, eperm = pgs.relabel(sc)
    g, r = dev_trial(capi, sc, False, lam), capi.pose_graph_debug_trial(*_args(rl), fix_scale=False, lam=lam)
    assert np.array_equal(r["e"], g["e"][eperm]) and np.array_equal(r["J"], g["J"][eperm])
    pgs.check_stages(r, rl, False, lam, f"device {rl['name']} lam={lam:g}", S_lin=pgs.normalise(rl["S"]))
    new_no = np.searchsorted(pgs.free_ids(rl), perm[pgs.free_ids(sc)])              # free-vertex number in the relabelled graph
    idx = (7 * new_no[:, None] + np.arange(7)[None, :]).ravel()
    H_back, b_back, x_back = np.tril(pgs.symmetric(r["H"])[np.ix_(idx, idx)]), r["b"][idx], r["x"][idx]
    ref = reference(g, sc)
    assert (np.abs(H_back - np.tril(g["H"])) <= pgs.h_bound(ref, lam)).all()
    assert (np.abs(b_back - g["b"]) <= (ref["bn"] + 2) * pgs.EPS * ref["babs"]).all()
    Hs = pgs.symmetric(ref["H"])
    keep = ref["Habs"].diagonal() > 0                 # (the lambda-only rows: see pg_scene.check_stages)
    x_ref = pgs.solve_ld(Hs[np.ix_(keep, keep)], ref["b"][keep], lam).astype(np.float64)
    xb, _ = pgs.x_bound(Hs[np.ix_(keep, keep)], lam, x_ref)
    assert np.abs(x_back - g["x"])[keep].max() <= xb and np.abs(x_back[keep] - x_ref).max() <= xb and not x_back[~keep].any()
    assert np.array_equal(r["vidx"] < 0, rl["fixed"] != 0)


def test_failure_flag(capi, oracle):
    """lambda = -1 on the clique: the tile Cholesky meets a non-positive pivot like the oracle's dense one -- the flag is set, x keeps
    its zeros, the estimates come back as they went in.  lambda = 1 on a component WITHOUT a fixed vertex (J^T J alone is singular there)
    is an ordinary solve that meets every stage bound."""
    sc = pgs.family("clique12")
    g = capi.pose_graph_debug_trial(*_args(sc), lam=-1.0)
    o = oracle.pose_graph_trial(*_args(sc), lam=-1.0)
    assert g["failed"] != 0 and o["failed"] != 0
    assert np.array_equal(g["S"], pgs.normalise(sc["S"])) and np.array_equal(o["S"], sc["S"]) and not g["x"].any() and not o["x"].any()
    assert np.abs(g["e"] - o["e"]).max() <= pgs.BOUND_E and np.abs(g["J"] - o["J"]).max() <= pgs.BOUND_J     # the stages before the solve stand
    fl = pgs.family("two_components16_floating")
    g = capi.pose_graph_debug_trial(*_args(fl), lam=1.0)
    assert g["failed"] == 0
    pgs.check_stages(g, fl, False, 1.0, "device floating component lam=1", S_lin=pgs.normalise(fl["S"]))


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_public_entry_point(capi, oracle, name, fix):
    """dvm_pose_graph_optimize for 20 iterations on the same graphs: the 'far' rule of test_gpu_ba.py::test_pose_graph_optimize with its
    tolerances (same trial counts and chi2 to 5e-5 while chi2 is above 1e-2 of the initial one), every fixed vertex bit-equal wherever it
    sits, the vertex without edges within 16 eps of where it started."""
    sc = pgs.family(name)
    So, sto = oracle.pose_graph_optimize(*_args(sc), fix_scale=fix, iterations=20)
    Sg, stg = capi.pose_graph_optimize(*_args(sc), fix_scale=fix, iterations=20)
    assert abs(stg["chi2_initial"] - sto[2]) <= 5e-5 * sto[2]
    far = [i for i in range(int(min(stg["iterations"], sto[0]))) if i == 0 or sto[6 + i] > 1e-2 * sto[2]]
    for i in far:
        assert stg["trials_per_iter"][i] == sto[38 + i], i
        assert abs(stg["chi2_per_iter"][i] - sto[6 + i]) <= 5e-5 * sto[6 + i], i
    Sn = pgs.normalise(sc["S"])
    fx = sc["fixed"] != 0
    assert np.array_equal(Sg[fx], Sn[fx]) and np.array_equal(So[fx], sc["S"][fx])
    if fix:
        assert np.array_equal(Sg[:, 7], Sn[:, 7])          # every update multiplies the scale by exp(0) = 1
    if name.startswith("isolated"):
        assert (np.abs(Sg[4] - Sn[4]) <= 16 * pgs.EPS * pgs.update_scale(Sn)[4]).all()


def test_rejected_trials_leave_the_linearisation_alone(capi, oracle):
    """Regression: the chi2-only pass at a trial state used to store its errors over the linearisation's, so every trial after a
    rejected one solved with b = -J^T e(rejected state).  chain8 with fix_scale: the second iteration rejects nine trials and accepts the
    tenth (rho = 0.54 in the oracle, 0.1151 -> 0.0528); the device rejected it.  A floating component with fix_scale: the first
    factorisation fails, and what the failed trial left behind made two runs of the same call differ."""
    sc = pgs.family("chain8")
    _, sto = oracle.pose_graph_optimize(*_args(sc), fix_scale=True, iterations=20)
    _, stg = capi.pose_graph_optimize(*_args(sc), fix_scale=True, iterations=20)
    assert list(sto[38:40]) == [1, 10] and list(stg["trials_per_iter"][:2]) == [1, 10]
    assert abs(stg["chi2_per_iter"][1] - sto[7]) <= 5e-5 * sto[7] and sto[7] < 0.5 * sto[6]
    fl = pgs.family("two_components16_floating")
    runs = [capi.pose_graph_optimize(*_args(fl), fix_scale=True, iterations=20) for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1]["chi2_per_iter"], runs[1][1]["chi2_per_iter"])
    assert list(runs[0][1]["trials_per_iter"]) == list(runs[1][1]["trials_per_iter"])


def test_public_entry_point_all_fixed(capi):
    """Every vertex fixed: nothing to optimise -- S comes back bit-equal and the statistics are zero."""
    sc = pgs.family("ring12")
    S, st = capi.pose_graph_optimize(sc["S0"], np.ones(len(sc["S0"]), np.uint8), sc["edges_v"], sc["edges_meas"], iterations=20)
    assert np.array_equal(S, sc["S0"])
    assert all(not np.any(v) for v in st.values())
    g = capi.pose_graph_debug_trial(sc["S0"], np.ones(len(sc["S0"]), np.uint8), sc["edges_v"], sc["edges_meas"], lam=1.0)
    assert g["nfree"] == 0 and (g["vidx"] == -1).all() and np.array_equal(g["S"], sc["S0"]) and g["failed"] == 0
