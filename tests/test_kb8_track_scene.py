"""Pins the scene of the KannalaBrandt8 tracked-frame tests (tests/kb8_track_scene.py) on the CPU, before any GPU sees it: the oracle's
extraction of the two frames (the device extractor's, bit for bit: tests/test_gpu_track_frame.py), SearchByProjection(CurrentFrame,
LastFrame) in kb8_scene.frames_ref's logic and kb8_scene.pose_kb8 on its edges."""
import numpy as np
import pytest

import kb8_scene as ks
import kb8_track_scene as kt


@pytest.fixture(scope="module")
def ref(oracle):
    orc = oracle.OrbOracle()
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    inv_s2 = (1.0 / (scale.astype(np.float64) ** 2)).astype(np.float32)
    return kt.reference(lambda im: orc.extract(im), scale, inv_s2)


def test_camera_covers_the_frame_inside_80_degrees():
    corners = np.array([[0, 0], [kt.COLS, 0], [0, kt.ROWS], [kt.COLS, kt.ROWS]], np.float32)
    rays = ks.unproject(kt.P, corners)
    theta = np.rad2deg(np.arctan2(np.hypot(rays[:, 0], rays[:, 1]), rays[:, 2]))
    assert 78.0 < theta.max() < 80.0, theta
    back = ks.project_f32(kt.P, rays)
    # (within 1e-4 px at the corner (0, 0); 640 and 480 have a float32 ulp of 6.1e-5 and 3.1e-5, and a corner there returns within two of them)
    assert np.abs(back[0] - corners[0]).max() < 1e-4 and np.abs(back - corners).max() <= 2 * np.spacing(np.float32(kt.COLS))
    pin = kt.P[0] * rays[:, :2] + kt.P[2:4]           # where a pinhole camera of the same fx puts those rays
    assert np.abs(pin - corners).max() > 800.0


def test_scene_tracks_and_tells_the_models_apart(ref):
    sc = ref
    assert (sc["mp_l"] >= 0).sum() > 500 and sc["nm"] >= 20, sc["nm"]
    planted = sc["planted"][sc["mp"][sc["sel"]]]       # per edge: its map point is a planted one
    outl = sc["outlier"].astype(bool)
    rest_rejected = int(outl[~planted].sum())
    print(f"seed {sc['seed']}: {sc['nm']} matches, {int(planted.sum())} planted edges, {rest_rejected} of {int((~planted).sum())} others rejected, "
          f"smallest |chi2 - 5.991| {sc['min_band']:.3g}")
    assert planted.sum() >= 10 and outl[planted].all()
    assert rest_rejected <= 0.05 * (~planted).sum()
    assert sc["min_band"] >= ks.CHI2_MARGIN
    # closer to the truth than the prediction, in translation and in rotation
    def rot(a, b):
        return 2.0 * np.arccos(min(1.0, abs(float(a[3:] @ b[3:])) / (np.linalg.norm(a[3:]) * np.linalg.norm(b[3:]))))
    gt, p0, T = sc["gt"], sc["pose0"], sc["pose"]
    assert np.linalg.norm(T[:3] - gt[:3]) < np.linalg.norm(p0[:3] - gt[:3])
    assert rot(T, gt) < rot(p0, gt)
    # the same edges on the pinhole camera K = p[0..3]: its rejections are not "the planted set and at most 5 % of the rest"
    pin = kt.pinhole_flags(sc).astype(bool)
    print(f"pinhole K on the same edges: {int(pin[planted].sum())} planted and {int(pin[~planted].sum())} others rejected")
    assert not (pin[planted].all() and pin[~planted].sum() <= 0.05 * (~planted).sum())
    assert not np.array_equal(pin, outl)
