"""The tile Cholesky on its own: dvm_tile_solve_debug hands the solver a linear system (tests/tile_scene.py) in every form the launcher has and
the x that comes back is compared with a long double solve.

Every solve is held to
  (a) the forward bound |x - x_ref|_inf <= 64 n eps cond |x_ref|_inf (pg_scene.x_bound's; cond: Gershgorin's bound for the diagonally dominant
      family, np.linalg.cond for the ill-conditioned one), and
  (b) the normwise residual eta = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf) <= RESIDUAL_FACTOR * max(eta of a float64 LAPACK Cholesky solve
      of the same system, eps).  What the reference shows (docs/NOTEBOOK.md section 42): LAPACK's eta sits at 0.0001 to 0.04 n eps on these
      systems, below eps itself up to n = 200, and moves by a factor of up to 3 between systems of one size and family (0.0011 to 0.0035
      n eps at n = 150 to 270).  The factor is that spread times 2.5 for the one thing the device does differently: the panel solves
      multiply by an explicit inverse of a 64 x 64 diagonal tile's factor instead of substituting.  It is a constant: it does not grow with
      the condition number, on the ill-conditioned family either.
Where the solver's file promises the same bits from two forms (its header: the level launches on every path, and the flow form), the bits
are compared; k_chol_pair and the raw-root panel solve sum in their own order and are held to (a) and (b)."""
import numpy as np
import pytest

import tile_scene as ts

pytestmark = pytest.mark.gpu
EPS = ts.EPS


RESIDUAL_FACTOR = 8


_cases = {}


def case(name, mask, n_blocks, dof=6, per_tile=10, kept_list=(), n_landmarks=0, seed=0, family="dominant", empty_tiles=()):
    """A system, its reference and what x holds before the solve; built once per name."""
    if name not in _cases:
        sh = ts.shape(n_blocks, dof, per_tile, kept_list, n_landmarks)
        sy = ts.dominant_system(mask, sh, seed, empty_tiles) if family == "dominant" else ts.ill_system(mask, sh, seed)
        x_ref = ts.solve_ref(sy["A"], sy["b"])
        x_in = np.random.default_rng(seed + 1000).uniform(1e3, 2e3, sh["x_len"])
        c = dict(name=name, sh=sh, mask=mask, sy=sy, x_ref=x_ref, x_in=x_in, eta_ref=ts.eta(sy["A"], sy["b"], ts.solve_f64(sy["A"], sy["b"])),
                 bound=ts.forward_bound(sy, x_ref))
        for v in (sy["A"], sy["b"], x_in):
            v.setflags(write=False)
        _cases[name] = c
    return _cases[name]


def solve(capi, c, form=0, **kw):
    sh = c["sh"]
    return capi.tile_solve_debug(kw.pop("A", c["sy"]["A"]), kw.pop("b", c["sy"]["b"]), sh["n_blocks"], sh["dof"], sh["per_tile"], kept_list=sh["kept_list"],
                                 n_landmarks=sh["n_landmarks"], mask=kw.pop("mask", c["mask"]), x_in=c["x_in"], form=form, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check(c, x, tag):
    """(a), (b) and the untouched rest of x for one solution; prints the figures docs/NOTEBOOK.md lists."""
    sh, sy = c["sh"], c["sy"]
    rest = np.ones(sh["x_len"], bool)
    rest[sh["x_index"]] = False
    assert (bits(x)[rest] == bits(c["x_in"])[rest]).all(), f"{c['name']} {tag}: x of a landmark that is not kept was written"
    xu = x[sh["x_index"]]
    assert np.isfinite(xu).all(), f"{c['name']} {tag}"
    err = float(np.abs(xu.astype(np.longdouble) - c["x_ref"]).max())
    eta = ts.eta(sy["A"], sy["b"], xu)
    n = sy["n"]
    print(f"TILE_SOLVE {c['name']:<22} {tag:<14} n {n:5d} cond {sy['cond']:9.3g} eta/(n eps) dev {eta / (n * EPS):8.4f} ref {c['eta_ref'] / (n * EPS):8.4f} "
          f"err/bound {err / c['bound']:.3g}")
    assert err <= c["bound"], f"{c['name']} {tag}: forward error {err:.3g} > {c['bound']:.3g}"
    limit = RESIDUAL_FACTOR * max(c["eta_ref"], EPS)
    assert eta <= limit, f"{c['name']} {tag}: eta {eta:.3g} > {limit:.3g}"


def forms(capi):
    return dict(level=capi.TILE_FORM_NO_PAIR, pair=0, flow=capi.TILE_FORM_FLOW | capi.TILE_FORM_NO_PAIR, per_phase=capi.TILE_FORM_NO_PAIR | capi.TILE_FORM_PER_PHASE)


def run_forms(capi, c, names):
    """Solves c in the named forms, checks each, returns {form: (x, info)}."""
    out = {}
    for k in names:
        x, fail, info = solve(capi, c, forms(capi)[k])
        assert fail[0] == 0, f"{c['name']} {k}"
        assert info["used_flow"] == (k == "flow")
        check(c, x[0], k)
        out[k] = (x[0], info)
    return out


def same_bits(res, a, b, name):
    assert (bits(res[a][0]) == bits(res[b][0])).all(), f"{name}: {a} and {b} differ in {(bits(res[a][0]) != bits(res[b][0])).sum()} words"


# ------------------------------------------------------------------------------------------------------------------ one tile, tile boundaries
@pytest.mark.parametrize("dof,per,nb", [(6, 10, 1), (6, 10, 2), (6, 10, 9), (6, 10, 10), (7, 9, 1), (7, 9, 8), (7, 9, 9)])
def test_one_tile(capi, dof, per, nb):
    """Every amount of identity padding in a single tile, 58 rows of it (one camera) included; the root's panel solve by the back
    substitution (n_root_raw) and launched (bound (a): the two sum in different orders, k_chol_backsolve)."""
    c = case(f"one_tile_{dof}x{nb}", ts.chain_mask(1), nb, dof, per, seed=nb)
    res = run_forms(capi, c, ["level", "per_phase", "flow"])
    assert res["level"][1]["level_path"][0] == "raw_root" and res["level"][1]["backsolve_cols"] == 1
    same_bits(res, "level", "per_phase", c["name"])
    x, fail, info = solve(capi, c, capi.TILE_FORM_NO_ROOT_RAW)
    assert fail[0] == 0 and info["level_path"][0] != "raw_root"
    check(c, x[0], "no_root_raw")


@pytest.mark.parametrize("nb", [11, 20, 21])
def test_tile_boundaries(capi, nb):
    c = case(f"boundary_{nb}", ts.chain_mask(-(-nb // 10)), nb, seed=nb)
    res = run_forms(capi, c, ["level", "pair", "flow"])
    same_bits(res, "level", "flow", c["name"])


# ------------------------------------------------------------------------------------------------------------------ pair, chains
def test_pair(capi):
    c = case("pair", ts.chain_mask(2), 17, seed=2)
    res = run_forms(capi, c, ["level", "pair", "flow", "per_phase"])
    ip, il = res["pair"][1], res["level"][1]
    assert ip["used_pair"] == 1 and set(ip["level_path"]) == {"none"} and ip["backsolve_cols"] == 0      # k_chol_pair alone
    assert il["used_pair"] == 0 and il["level_path"][0] != "none" and il["level_path"][1] == "raw_root" and il["backsolve_cols"] == 2
    same_bits(res, "level", "flow", "pair")
    same_bits(res, "level", "per_phase", "pair")
    assert np.abs(res["pair"][0] - res["level"][0]).max() <= c["bound"]      # k_chol_pair sums in its own order: within (a) of the level launches


@pytest.mark.parametrize("tiles,nb", [(3, 25), (4, 40)])
def test_chains(capi, tiles, nb):
    """The pair on top of level launches; n_root_raw honoured and zero."""
    c = case(f"chain_{tiles}", ts.chain_mask(tiles), nb, seed=tiles)
    res = run_forms(capi, c, ["level", "pair", "flow", "per_phase"])
    ip = res["pair"][1]
    assert ip["used_pair"] == 1 and (ip["pair_a"], ip["pair_b"]) == (tiles - 2, tiles - 1)
    assert all(p != "none" for p in ip["level_path"][:tiles - 2]) and set(ip["level_path"][tiles - 2:]) == {"none"} and ip["backsolve_cols"] == tiles - 2
    same_bits(res, "level", "flow", c["name"])
    same_bits(res, "level", "per_phase", c["name"])
    x, fail, info = solve(capi, c, capi.TILE_FORM_NO_PAIR | capi.TILE_FORM_NO_ROOT_RAW)
    assert fail[0] == 0 and "raw_root" not in info["level_path"] and "raw_root" in res["level"][1]["level_path"]
    check(c, x[0], "no_root_raw")
    x, fail, info = solve(capi, c, capi.TILE_FORM_NO_PAIR | capi.TILE_FORM_NO_DIAG_IN_LEVEL)
    assert fail[0] == 0 and not {"level_one_launch", "slices_diag_update"} & set(info["level_path"])
    check(c, x[0], "no_diag_in_lvl")
    assert (bits(x[0]) == bits(res["level"][0])).all()


def test_ill_conditioned(capi):
    """cond about 1e9, as a bundle adjustment's reduced system at small lambda: the residual (b) keeps its constant factor here, so a panel
    solve that loses accuracy with the conditioning shows; bound (a) takes np.linalg.cond."""
    for tiles, nb, dof, per in [(2, 15, 6, 10), (3, 25, 6, 10), (3, 22, 7, 9)]:
        c = case(f"ill_{dof}_{tiles}", ts.chain_mask(tiles), nb, dof, per, seed=tiles, family="ill")
        res = run_forms(capi, c, ["level", "pair", "flow"])
        same_bits(res, "level", "flow", c["name"])


# ------------------------------------------------------------------------------------------------------------------ arrow: the launcher's level paths
def test_arrow_paths(capi):
    """Leaf counts on either side of the launcher's three thresholds, from the schedule's own counts: the four level paths by name, each with
    the bits of the per-phase form, and the flow form on the same systems."""
    arrows = ts.arrow_leaf_counts(capi.tile_schedule_debug)
    seen = set()
    for k, want in sorted(arrows.items()):
        c = case(f"arrow_{k}", ts.arrow_mask(k), 10 * k + 3, seed=k)
        res = run_forms(capi, c, ["level", "per_phase", "flow"])
        info = res["level"][1]
        assert info["level_nc"][0] == k and info["level_path"][:2] == [want, "raw_root"], (k, info["level_path"])
        assert res["per_phase"][1]["level_path"][0] == "diag_trsm_update"
        same_bits(res, "level", "per_phase", c["name"])
        same_bits(res, "level", "flow", c["name"])
        seen.add(info["level_path"][0])
    assert seen == {"level_one_launch", "slices_diag_update", "diag_fused", "diag_trsm_update"}


# ------------------------------------------------------------------------------------------------------------------ flow form, masks
MASKS = [("bush", ts.bush_mask, 66), ("dense_4", lambda: ts.dense_mask(4), 33)] + \
        [(f"random_{t}_{s}", (lambda t=t, s=s: ts.random_mask(t, s)), 10 * t - 4) for t, s in ts.RANDOM_MASKS]


@pytest.mark.parametrize("name,mask,nb", MASKS, ids=[m[0] for m in MASKS])
def test_masks_level_and_flow(capi, name, mask, nb):
    c = case(name, mask(), nb, seed=nb)
    res = run_forms(capi, c, ["level", "pair", "flow", "per_phase"])
    same_bits(res, "level", "flow", name)
    same_bits(res, "level", "per_phase", name)
    if res["pair"][1]["pair_a"] < 0:
        same_bits(res, "level", "pair", name)


def test_structurally_present_empty_tile(capi):
    """A tile the mask has and the matrix leaves at zero, and the mask derived from the matrix (which then has no such tile)."""
    c = case("empty_tile", ts.dense_mask(3), 30, seed=7, empty_tiles=[(2, 0)])
    run_forms(capi, c, ["level", "pair", "flow"])
    x, fail, info = solve(capi, c, mask=None)
    assert fail[0] == 0
    check(c, x[0], "derived_mask")


def test_two_roots_refused_by_flow(capi):
    c = case("two_trees", ts.two_trees_mask(), 45, seed=9)
    res = run_forms(capi, c, ["level", "per_phase"])
    same_bits(res, "level", "per_phase", "two_trees")
    assert res["level"][1]["roots"] == 2 and res["level"][1]["flow_refusal"] & 2
    with pytest.raises(capi.DvmError, match="does not admit"):
        solve(capi, c, capi.TILE_FORM_FLOW)


@pytest.mark.parametrize("name,mask,nb", [("sim3_chain", lambda: ts.chain_mask(3), 22), ("sim3_bush", ts.bush_mask, 60)])
def test_sim3_layout_in_ba_forms(capi, name, mask, nb):
    """(7, 9) through the forms the pose graph never uses: pair, in-launch hand-offs, flow."""
    c = case(name, mask(), nb, 7, 9, seed=nb)
    res = run_forms(capi, c, ["level", "pair", "flow", "per_phase"])
    same_bits(res, "level", "flow", name)
    same_bits(res, "level", "per_phase", name)
    assert res["pair"][1]["used_pair"] == (name == "sim3_chain")


# ------------------------------------------------------------------------------------------------------------------ kept landmarks
@pytest.mark.parametrize("n_kept", [1, 21, 22, 43])
def test_kept_landmarks(capi, n_kept):
    """kept_list neither monotone nor dense in a larger n_landmarks; x of every other landmark keeps its bits (check)."""
    rng = np.random.default_rng(n_kept)
    kept = rng.permutation(3 * n_kept + 5)[:n_kept]
    kt = -(-n_kept // 21)
    mask = ts.with_kept(ts.chain_mask(3), kt, [(k, c) for k in range(kt) for c in (0, 2)] + [(kt - 1, 1)])
    c = case(f"kept_{n_kept}", mask, 24, kept_list=kept, n_landmarks=3 * n_kept + 5, seed=n_kept)
    assert n_kept == 1 or (np.diff(kept) < 0).any()
    res = run_forms(capi, c, ["level", "pair", "flow", "per_phase"])
    same_bits(res, "level", "flow", c["name"])
    same_bits(res, "level", "per_phase", c["name"])


# ------------------------------------------------------------------------------------------------------------------ repeats
@pytest.mark.parametrize("form", ["level", "pair", "flow"])
def test_repeats(capi, form):
    """The hand-off flags compare against the solve's sequence number: three solves on one structure give the same bits, with another system
    solved in between as well."""
    c = case("bush", ts.bush_mask(), 66, seed=66)
    other = ts.dominant_system(c["mask"], c["sh"], seed=4242)
    x, fail, _ = solve(capi, c, forms(capi)[form], repeats=3)
    assert not fail.any() and (bits(x[1]) == bits(x[0])).all() and (bits(x[2]) == bits(x[0])).all()
    check(c, x[0], f"repeat_{form}")
    y, fail, info = solve(capi, c, forms(capi)[form], repeats=3, A2=other["A"], b2=other["b"])
    assert not fail.any() and not info["fail2"].any()
    assert (bits(y) == bits(x)).all()
    assert (bits(info["x2"][0]) == bits(info["x2"][1])).all() and (bits(info["x2"][0]) != bits(x[0])).any()
    oc = dict(c, name="bush_other", sy=other, x_ref=ts.solve_ref(other["A"], other["b"]), eta_ref=ts.eta(other["A"], other["b"], ts.solve_f64(other["A"], other["b"])))
    oc["bound"] = ts.forward_bound(other, oc["x_ref"])
    check(oc, info["x2"][0], f"between_{form}")


# ------------------------------------------------------------------------------------------------------------------ failure
FAIL_ROWS = (0, 15, 16, 47, 48, 59)


def _fail_structures(capi):
    chain = case("fail_chain", ts.chain_mask(4), 40, seed=40)
    kept = case("fail_kept", ts.with_kept(ts.chain_mask(3), 1, [(0, 0), (0, 2)]), 30, kept_list=np.arange(21)[::-1], n_landmarks=21, seed=41)
    info = capi.tile_schedule_debug(chain["mask"])
    assert (info["pair_a"], info["pair_b"]) == (2, 3)
    return {"leaf": (chain, 0), "interior": (chain, 1), "pair_a": (chain, info["pair_a"]), "pair_b": (chain, info["pair_b"]), "kept": (kept, 3)}


@pytest.mark.parametrize("where", ["leaf", "interior", "pair_a", "pair_b", "kept"])
@pytest.mark.parametrize("form", ["level", "pair", "flow"])
def test_failure(capi, where, form):
    """The first non-positive pivot at rows 0, 15, 16, 47, 48 and 59 (each 16-column panel, first and last column) of a leaf column, an
    interior column (in the flow form: a column its chain climbs to), the pair's two columns and a kept-landmark tile; negative, NaN and, at
    row 0 of the leaf, exactly zero.  Ordinary inputs with a defined answer: the fail word is set and x keeps every bit it held; the good
    system solved on the same structure afterwards meets (a) and (b) and has the bits of the solve before."""
    c, tile = _fail_structures(capi)[where]
    A = c["sy"]["A"]
    if "pivots" not in c:
        c["pivots"] = ts.pivots_ld(A)
    first = None
    for trow in FAIL_ROWS:
        r = ts.unknown_row(c["sh"], tile, trow)
        for kind in ("negative", "nan") + (("zero",) if (where, trow) == ("leaf", 0) else ()):
            B = ts.break_pivot(A, c["pivots"], r, kind)
            x, fail, info = solve(capi, c, forms(capi)[form], repeats=2, A2=B, b2=c["sy"]["b"])
            tag = f"{where} row {trow} {kind} {form}"
            assert info["fail2"][0] != 0, tag
            assert (bits(info["x2"][0]) == bits(c["x_in"])).all(), f"{tag}: a failed solve wrote {(bits(info['x2'][0]) != bits(c['x_in'])).sum()} words of x"
            assert info["used_pair"] == (form == "pair") and info["used_flow"] == (form == "flow"), tag
            assert not fail.any() and (bits(x[1]) == bits(x[0])).all(), tag
            if first is None:
                first = x[0]
                check(c, x[1], f"after_{where}_{form}")
            assert (bits(x[0]) == bits(first)).all(), tag      # every good solve, before and after every failure, is the one checked
