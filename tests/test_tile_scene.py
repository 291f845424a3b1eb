"""tests/tile_scene.py checked on the CPU: the layout against values written out by hand, the two references against each other, the
condition bounds, the position of the broken pivots, and -- from the schedule alone (dvm_tile_schedule_debug, host only) -- which masks reach
which form of the solve."""
import numpy as np
import pytest

import tile_scene as ts


def test_layout_by_hand():
    sh = ts.shape(12, 6, 10, kept_list=[7, 2, 30] + list(range(8, 27)), n_landmarks=40)      # 22 kept: two kept tiles behind two camera tiles
    assert (sh["ncamt"], sh["tiles"], sh["n"], sh["x_len"]) == (2, 4, 72 + 66, 72 + 120)
    rows, xi = sh["rows"], sh["x_index"]
    assert list(rows[:7]) == [0, 1, 2, 3, 4, 5, 6] and rows[59] == 59            # block 9 ends at row 59: rows 60..63 are padding
    assert rows[60] == 64 and rows[71] == 75                                     # block 10 opens tile 1
    assert rows[72] == 128 and rows[72 + 62] == 128 + 62                         # kept 0..20 fill rows 0..62 of tile 2 (row 63: padding)
    assert rows[72 + 63] == 192 and rows[72 + 65] == 194                         # kept 21 opens tile 3
    assert list(xi[:3]) == [0, 1, 2] and xi[71] == 71
    assert list(xi[72:78]) == [72 + 21, 72 + 22, 72 + 23, 72 + 6, 72 + 7, 72 + 8]   # kept 0 = landmark 7, kept 1 = landmark 2
    assert xi[72 + 6] == 72 + 90                                                  # kept 2 = landmark 30
    s7 = ts.shape(10, 7, 9)
    assert s7["rows"][62] == 62 and s7["rows"][63] == 64 and s7["tiles"] == 2 and s7["x_len"] == 70   # 9 Sim3 blocks = 63 rows, row 63 padding
    x = ts.expand(sh, np.arange(1, sh["n"] + 1), np.full(sh["x_len"], -1.0))
    assert x[72 + 3 * 7] == 73 and x[72 + 3 * 2] == 76 and x[72] == -1 and (x == -1).sum() == 120 - 66
    assert ts.unknown_row(sh, 2, 59) == 72 + 59 and ts.unknown_row(sh, 1, 11) == 71


SMALL = [(1, 1), (2, 11), (3, 25), (4, 40)]     # (tiles of a chain, blocks)


@pytest.mark.parametrize("tiles,nb", SMALL)
def test_references_agree_and_bounds_hold(tiles, nb):
    sh = ts.shape(nb)
    sy = ts.dominant_system(ts.chain_mask(tiles), sh, seed=nb)
    A = sy["A"]
    assert (A == A.T).all()
    d = np.diag(A)
    assert (np.abs(A).sum(axis=1) - d <= d / 2).all()
    assert np.linalg.cond(A) <= sy["cond"]
    x1, x2 = ts.solve_ref(A, sy["b"]), ts.solve_refined(A, sy["b"])
    assert np.abs(x1 - x2).max() <= 2.0 ** -55 * np.abs(x1).max()
    tile_of = sh["tile_of"]
    assert not A[np.abs(tile_of[:, None] - tile_of[None, :]) > 1].any()          # nothing outside the chain's tiles


def test_empty_tile_stays_empty():
    sh = ts.shape(30)
    sy = ts.dominant_system(ts.dense_mask(3), sh, seed=3, empty_tiles=[(2, 0)])
    t = sh["tile_of"]
    assert not sy["A"][np.ix_(t == 2, t == 0)].any() and sy["A"][np.ix_(t == 2, t == 1)].any()


@pytest.mark.parametrize("tiles,nb,dof,per", [(2, 15, 6, 10), (3, 25, 6, 10), (3, 22, 7, 9)])
def test_ill_family_condition(tiles, nb, dof, per):
    sy = ts.ill_system(ts.chain_mask(tiles), ts.shape(nb, dof, per), seed=tiles)
    assert 1e8 <= sy["cond"] <= 1e10
    assert (sy["A"] == sy["A"].T).all()


def test_broken_pivot_sits_where_asked():
    sh = ts.shape(40)
    A = ts.dominant_system(ts.chain_mask(4), sh, seed=5)["A"]
    d = ts.pivots_ld(A)
    assert len(d) == len(A) and (d > 0).all()
    for tile, trow, kind in [(0, 0, "zero"), (0, 0, "negative"), (1, 15, "negative"), (2, 16, "nan"), (3, 59, "negative"), (2, 47, "negative"), (1, 48, "nan")]:
        r = ts.unknown_row(sh, tile, trow)
        B = ts.break_pivot(A, d, r, kind)
        assert (B != A).sum() == 1
        bad = ts.pivots_ld(B)
        assert len(bad) == r + 1 and not bad[r] > 0 and (bad[:r] > 0).all(), (tile, trow, kind)
        if kind == "zero":
            assert bad[r] == 0


def test_masks_reach_their_forms(capi):
    sched = capi.tile_schedule_debug
    one = sched(ts.chain_mask(1))
    assert (one["levels"], one["pair_a"], one["n_root_raw"], one["roots"]) == (2, -1, 1, 1)
    for t in (2, 3, 4):
        c = sched(ts.chain_mask(t))
        assert (c["pair_a"], c["pair_b"], c["n_root_raw"], c["flow_leaves"]) == (t - 2, t - 1, 1, 1) and not c["flow_refusal"] & capi.TILE_FLOW_REFUSED
    bush = sched(ts.bush_mask())
    assert bush["level_nc"] == [4, 2, 1, 1] and bush["pair_a"] == -1 and bush["roots"] == 1
    two = sched(ts.two_trees_mask())
    assert two["roots"] == 2 and two["flow_refusal"] & 2
    # the arrow's leaf counts on either side of the launcher's three thresholds, and the four level paths they stand for
    arrows = ts.arrow_leaf_counts(sched)
    assert len(arrows) == 5 and set(arrows.values()) == {"level_one_launch", "slices_diag_update", "diag_fused", "diag_trsm_update"}
    assert max(arrows) <= 64 and not sched(ts.arrow_mask(max(arrows)))["flow_refusal"] & capi.TILE_FLOW_REFUSED
    # with fewer workgroups than four per leaf the admission test refuses
    assert sched(ts.arrow_mask(max(arrows)), workgroups=4 * max(arrows) - 1)["flow_refusal"] & 4


def test_random_masks_stay_in_coverage(capi):
    """Every seeded mask is solved in the level form; at most a quarter may be out of the flow form's reach."""
    refused = 0
    for t, seed in ts.RANDOM_MASKS:
        m = ts.random_mask(t, seed)
        assert m.shape == (t, t) and 6 <= t <= 14 and (np.triu(m, 1) == 0).all()
        refused += bool(capi.tile_schedule_debug(m)["flow_refusal"] & capi.TILE_FLOW_REFUSED)
    assert 4 * refused <= len(ts.RANDOM_MASKS)
