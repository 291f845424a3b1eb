"""Pins the scenes of tests/test_gpu_fuse_targets.py with pyoracle.project_search alone, so that the GPU parity tests cannot pass
vacuously: every pinned (seed, T, N) has enough hits and shows every way a (target, point) pair can end -- each of Fuse's gates, an empty
window, a best distance above TH_LOW, and a candidate the 5.99 gate dropped although its descriptor beats the returned best.  The
smaller N of the GPU tests are prefixes of these scenes' point tables."""
import numpy as np
import pytest

import fuse_targets_scene as fts
from dvm_slam_amd import synth

PINNED = [(0, 5, 200), (1, 33, 200), (2, 2, 200), (3, 1, 200)]     # (seed, T, N): the scenes of the GPU tests


def _reject_reasons(kf, pts):
    """Why Fuse's gates reject a point, in the reference's order, in float64 -- only clear-cut cases are counted."""
    R, t = synth.Rt_from_se3(kf["Tcw"])
    X = pts["pos"].astype(np.float64)
    Xc = X @ R.T + t
    Ow = -R.T @ t
    with np.errstate(divide="ignore", invalid="ignore"):
        u = 500.0 * Xc[:, 0] / Xc[:, 2] + 320.0; v = 500.0 * Xc[:, 1] / Xc[:, 2] + 240.0
    d = np.linalg.norm(X - Ow, axis=1)
    behind = Xc[:, 2] < -1e-3
    front = Xc[:, 2] > 1e-3
    outside = front & ((u < -1) | (u > 641) | (v < -1) | (v > 481))
    inside = front & (u > 1) & (u < 639) & (v > 1) & (v < 479)
    off_range = inside & ((d < 0.79 * pts["min_dist"]) | (d > 1.21 * pts["max_dist"]))
    in_range = inside & (d > 0.81 * pts["min_dist"]) & (d < 1.19 * pts["max_dist"])
    angle = in_range & (np.einsum("ij,ij->i", X - Ow, pts["normal"].astype(np.float64)) < 0.49 * d)
    return behind, outside, off_range, angle


@pytest.mark.parametrize("seed,T,N", PINNED)
def test_scene_is_not_vacuous(seed, T, N):
    sc = fts.prefix(fts.scene(seed, T), N)
    pts, skip = sc["pts"], sc["skip"]
    bi, bd = fts.oracle_rows(sc["targets"], pts, skip)
    unmasked = (pts["valid"][None, :] != 0) & (skip == 0)
    assert np.all(bi[~unmasked] == -1) and np.all(bd[~unmasked] == 256)                 # a masked entry reads "none"
    assert (bi >= 0).sum() >= 0.25 * unmasked.sum(), ((bi >= 0).sum(), unmasked.sum())
    seen = dict(behind=0, outside=0, off_range=0, angle=0, empty_window=0, above_th_low=0, gate_beats_best=0)
    for t, kf in enumerate(sc["targets"]):
        v = unmasked[t]
        _, d_gate, proj = fts.oracle_target(kf, pts, v)
        _, d_free, _ = fts.oracle_target(kf, pts, v, gate=False)
        rejected = v & (proj[:, 3] < 0)
        for name, m in zip(("behind", "outside", "off_range", "angle"), _reject_reasons(kf, pts)):
            seen[name] += int((m & rejected).sum())
            assert not np.any(m & v & (proj[:, 3] >= 0)), name                           # a clear-cut reject is rejected
        searched = v & (proj[:, 3] >= 0)
        seen["empty_window"] += int((searched & (d_free == 256)).sum())
        seen["above_th_low"] += int((searched & (d_gate > 50) & (d_gate < 256)).sum())
        seen["gate_beats_best"] += int((searched & (d_free < d_gate)).sum())
        assert np.all(d_free <= d_gate)
    assert all(n >= 1 for n in seen.values()), seen


def test_scene_variants():
    sc = fts.scene(0, 5)
    sizes = [len(kf["kps"]) for kf in sc["targets"]]
    assert sizes[fts.EMPTY_TARGET] == 0 and sizes[-1] == fts.BIG_TARGET_KEYPOINTS and len(set(sizes)) == 5 and all(s <= 300 for s in sizes[:-1])
    sizes = [len(kf["kps"]) for kf in fts.scene(1, 33)["targets"]]
    assert sizes[fts.EMPTY_TARGET] == 0 and sizes[-1] == fts.BIG_TARGET_KEYPOINTS and min(sizes[2:]) >= 150
    # a pair of points that best-matches the same keypoint of one target
    bi, _ = fts.oracle_rows(sc["targets"], sc["pts"], None, use_valid=False)
    shared = 0
    for row in bi:
        hit = row[row >= 0]
        shared += len(hit) - len(np.unique(hit))
    assert shared >= 1
    # the empty target finds nothing; a prefix is the same scene
    assert np.all(bi[fts.EMPTY_TARGET] == -1)
    b17, _ = fts.oracle_rows(sc["targets"], fts.prefix(sc, 17)["pts"], None, use_valid=False)
    assert np.array_equal(b17, bi[:, :17])
