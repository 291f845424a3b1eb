"""The scenes of tests/test_gpu_ba_window_fast_kb8.py, pinned on the CPU: tests/ba_kb8_window_scene.py draws what tests/ba_kb8_scene.py draws,
its two new shapes have an admissible seed under both fisheye cameras, and its recorded theta-ulp movement is what this machine measures."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import ba_kb8_scene as bs  # noqa: E402
import ba_kb8_window_scene as ws  # noqa: E402


@pytest.mark.parametrize("case", ["a", "d"])
@pytest.mark.parametrize("model", ["robomaster", "tum", "pinhole"])
def test_generator_is_ba_scene(model, case):
    for seed in (0, 3):
        a, b = bs.ba_scene(model, case, seed), ws.scene(model, bs.CASES[case], seed)
        for key in ("poses0", "fixed", "points0", "edges", "bad", "nudge", "poses_gt", "points_gt", "n_obs"):
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (key, seed)


def test_shapes_are_the_five_cases_and_two_more():
    assert {k: ws.SHAPES[k] for k in bs.CASES} == bs.CASES and set(ws.SHAPES) - set(bs.CASES) == set(ws.NEW_SHAPES)
    assert ws.SHAPES["w30"] == (32, 2, 300, 2500) and ws.SHAPES["w1"] == (4, 3, 64, 215)
    assert len(ws.window_cases()) == 14


@pytest.mark.parametrize("name", ws.NEW_SHAPES)
@pytest.mark.parametrize("model", bs.MODELS)
def test_new_shape_has_an_admissible_seed(model, name):
    sc, ref, seed = ws.case(model, name)
    P, n_fixed, L, E = ws.SHAPES[name]
    assert sc["poses0"].shape == (P, 7) and sc["points0"].shape == (L, 3) and len(sc["edges"]) == E and int(sc["fixed"].sum()) == n_fixed
    used = np.zeros(P, bool); used[sc["edges"]["pose"]] = True
    assert int((used & (sc["fixed"] == 0)).sum()) == P - n_fixed          # every free camera is observed: w30 has 30, w1 has one
    assert ref["admissible"] and ref["trials"] == ref["trials_n"] and ref["stop"] == ref["stop_n"]
    assert len(ref["trials"]) >= 3 and ref["dchi2"] > 0.0
    assert float(np.min(np.abs(ref["chi2"] - bs.CHI2_MONO))) >= bs.BAND_FACTOR * ref["dchi2"]
    print(f"{model} {name}: seed {seed}, trials {ref['trials']}, stop {ref['stop']}, ulp moves poses {ref['dpose']:.2e} points {ref['dpoint']:.2e} chi2 {ref['dchi2']:.2e}")


def test_old_shapes_come_from_ba_kb8_scene():
    assert ws.case("tum", "d")[0] is bs.ba_case("tum", "d")[0]
    assert ws.pinhole_twin("a", 0) is bs.ba_scene("pinhole", "a", 0)


def test_over_capacity_shape_has_31_free_cameras():
    sc = ws.scene("robomaster", ws.OVER_CAPACITY, 0)
    used = np.zeros(len(sc["poses0"]), bool); used[sc["edges"]["pose"]] = True
    assert int((used & (sc["fixed"] == 0)).sum()) == 31


def test_theta_ulp_tolerance_matches_the_record():
    dp, dx = ws.theta_ulp_window_diff()
    print(f"theta ulp, 14 window scenes: poses {dp:.3e} (recorded {ws.THETA_ULP_WIN_POSE_DIFF:.3e}), points {dx:.3e} (recorded {ws.THETA_ULP_WIN_POINT_DIFF:.3e})")
    assert 0.5 * ws.THETA_ULP_WIN_POSE_DIFF <= dp <= ws.THETA_ULP_WIN_POSE_DIFF
    assert 0.5 * ws.THETA_ULP_WIN_POINT_DIFF <= dx <= ws.THETA_ULP_WIN_POINT_DIFF
