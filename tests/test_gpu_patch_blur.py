"""GPU parity of the throughput path's descriptor kernel that blurs each keypoint's own patch (k_orient_desc_blur, DVM_PATCH_BLUR=1)
against the blurred-pyramid path (k_blur7 + k_orient_desc, DVM_PATCH_BLUR=0) and against the CPU oracle.

Every comparison is bitwise: the patch blur runs the tile blur's fixed-point arithmetic (blur_tile.h) on the same raw pixels.

A batch has one image size, so "the five frames" of the first check are spread over three batches of five, one per size: each holds the
textured frame(s) of its size, a flat frame (0 keypoints) and a frame with a single corner.  Five frames put a batch on the throughput
path (more than kLatencyBatch = 4) with three padding frames in the kernels' frame map (frames come in groups of eight).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KP_PER_WG = 16     # k_orient_desc_blur: four waves x kPbPerWave = 4 keypoints per workgroup
B = 5
# 150 x 200 small_image seeds, chosen on the CPU with the oracle (the tests assert what each was chosen for):
SEED_FRAME = 313   # level-0 keypoints at cx = 19, cx = w - 20, cy = 19 and cy = h - 20; patches reaching the mirrored frame on >= 3 higher levels
SEED_ONE = 301     # 401 keypoints: exactly one in the last workgroup
SEED_RAGGED = 303  # 420 keypoints: four in the last workgroup
EDGE_SHAPE = (150, 200)


def _same(res_a, res_b, what):
    (n_a, k_a, d_a, m_a), (n_b, k_b, d_b, m_b) = res_a, res_b
    assert (n_a, m_a) == (n_b, m_b), what
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(k_a[f], k_b[f]), (what, f)
    assert np.array_equal(d_a, d_b), what


def _extractor(capi, switch, max_batch=B):
    """A handle of its own: the switch is read once, when the handle is created."""
    old = os.environ.get("DVM_PATCH_BLUR")
    os.environ["DVM_PATCH_BLUR"] = switch
    try:
        return capi.OrbExtractor(max_batch=max_batch)
    finally:
        if old is None:
            del os.environ["DVM_PATCH_BLUR"]
        else:
            os.environ["DVM_PATCH_BLUR"] = old


def _corner(h, w):
    """One bright quadrant: a single corner, which FAST finds on a few of the resized levels (7, 3 and 1 keypoints at the three sizes)."""
    img = np.full((h, w), 127, np.uint8)
    img[h // 3:, w // 2:] = 255
    return img


def _batch(shape, frames):
    from dvm_slam_amd import synth
    h, w = shape
    if shape == (480, 640):
        tex = [frames[0], frames[1], frames[2]]
    else:
        tex = [synth.small_image(11 + k, h, w) for k in range(3)]
    return np.stack([tex[0], np.full((h, w), 127, np.uint8), tex[1], _corner(h, w), tex[2]])


@pytest.fixture(scope="module")
def edge_batch(oracle):
    """The 150 x 200 batch of the frame, tail, lazy-blur and second-call tests, with the oracle's results, computed once."""
    from dvm_slam_amd import synth
    imgs = np.stack([synth.small_image(s, *EDGE_SHAPE) for s in (SEED_FRAME, SEED_ONE, 305, SEED_RAGGED, 306)])
    orc = oracle.OrbOracle()
    return imgs, [orc.extract(im) for im in imgs]


@pytest.fixture(scope="module")
def edge_fused(capi, edge_batch):
    imgs, _ = edge_batch
    e = _extractor(capi, "1")
    e.extract_batch_host(imgs)
    res = [e.download(f) for f in range(B)]
    yield e, res
    e.close()


@pytest.mark.parametrize("shape", [(480, 640), (120, 160), (97, 131)])
def test_both_paths_equal_each_other_and_the_oracle(capi, oracle, frames, shape):
    imgs = _batch(shape, frames)
    orc = oracle.OrbOracle()
    ref = [orc.extract(im) for im in imgs]
    assert ref[1][0] == 0 and ref[3][0] >= 1 and ref[0][0] > KP_PER_WG, [r[0] for r in ref]
    got = {}
    for switch in ("1", "0"):
        e = _extractor(capi, switch)
        e.profiling(True)
        e.extract_batch_host(imgs)
        got[switch] = [e.download(f) for f in range(B)]
        # the switch does what it says: the fused path launches no blur at all
        assert (e.profile_get("blur")[1] == 0) == (switch == "1"), switch
        assert e.profile_get("orient_desc")[1] >= 1
        e.close()
    for f in range(B):
        _same(got["1"][f], got["0"][f], (shape, f, "fused vs blurred pyramid"))
        _same(got["1"][f], ref[f], (shape, f, "fused vs oracle"))
        _same(got["0"][f], ref[f], (shape, f, "blurred pyramid vs oracle"))


def test_keypoints_at_the_frame_of_a_level(oracle, edge_batch, edge_fused):
    imgs, ref = edge_batch
    h, w = EDGE_SHAPE
    orc = oracle.OrbOracle()
    orc.extract(imgs[0])
    k0 = orc.level_keypoints(0)
    x, y = k0["x"].astype(int), k0["y"].astype(int)
    assert (x == 19).any() and (x == w - 20).any() and (y == 19).any() and (y == h - 20).any()
    reaching = 0   # higher levels with a keypoint whose 43 x 43 raw patch leaves the level's interior
    for l in range(1, 8):
        kl = orc.level_keypoints(l)
        lh, lw = orc.level_dims(l)
        xx, yy = kl["x"].astype(int), kl["y"].astype(int)
        reaching += bool(((xx < 21) | (xx > lw - 22) | (yy < 21) | (yy > lh - 22)).any())
    assert reaching >= 3
    _same(edge_fused[1][0], ref[0], "frame keypoints")


def test_tails(edge_batch, edge_fused):
    _, ref = edge_batch
    assert ref[1][0] % KP_PER_WG == 1            # exactly one keypoint in the last workgroup
    assert ref[3][0] % KP_PER_WG not in (0, 1)   # a ragged last workgroup
    for f in range(B):
        _same(edge_fused[1][f], ref[f], ("tail", f))


def test_lazy_debug_blur(oracle, edge_batch, edge_fused):
    """After a fused batch no blurred pyramid exists: dvm_orb_debug_blurred makes it on demand, for any frame of the batch."""
    imgs, ref = edge_batch
    e, _ = edge_fused
    orc = oracle.OrbOracle()
    for f in (0, B - 1):
        orc.extract(imgs[f])
        levels = 0
        for l in range(8):
            bo = orc.blurred(l)
            if bo is not None:
                assert np.array_equal(e.debug_blurred(f, l), bo), (f, l)
                levels += 1
        assert levels >= 4
    for f in range(B):   # the results of the batch are untouched by it
        _same(e.download(f), ref[f], ("after debug_blurred", f))


def test_second_call_on_the_same_handle(capi, oracle, edge_batch):
    """Buffers are reused and the blurred pyramid is stale again after every fused batch."""
    from dvm_slam_amd import synth
    imgs_a, ref_a = edge_batch
    imgs_b = np.stack([synth.small_image(500 + k, *EDGE_SHAPE) for k in range(B)])
    orc = oracle.OrbOracle()
    ref_b = [orc.extract(im) for im in imgs_b]   # (orc now holds the last frame of b)
    e = _extractor(capi, "1")
    e.extract_batch_host(imgs_a)
    for f in range(B):
        _same(e.download(f), ref_a[f], ("first call", f))
    assert e.debug_blurred(0, 0).any()           # fills the blurred pyramid from batch a ...
    e.extract_batch_host(imgs_b)
    for f in range(B):
        _same(e.download(f), ref_b[f], ("second call", f))
    for l in range(8):                           # ... which must not be what the getter returns for batch b
        bo = orc.blurred(l)
        if bo is not None:
            assert np.array_equal(e.debug_blurred(B - 1, l), bo), l
    e.close()
