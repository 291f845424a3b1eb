"""GPU parity of the throughput path's pyramid kernel that loads its source bytes straight from global memory (k_pyr_resize_direct,
DVM_PYR_DIRECT=1) against the LDS-tile kernel (k_pyr_resize, DVM_PYR_DIRECT=0) and against the CPU oracle.  Bitwise throughout.

Batches hold nine frames: the smallest batch on the throughput resize path (more than kRzLatencyBatch = 8).  Eight come from
synth.small_image, frame 4 is flat.  dvm_orb_debug_pyr_path is asserted for every level, so that a silent fallback to the old kernel
cannot pass for the new one; which levels qualify is restated in tests/pyr_direct_model.py (strip_rows)."""
import os

import numpy as np
import pytest

import pyr_direct_model as model

pytestmark = pytest.mark.gpu

B = 9
# (rows, cols), scale factor, levels, what the case is there for
CASES = [
    ((97, 131), 1.2, 8),     # ragged last strip, odd widths, a tiny level 7 (k_pyr_resize + k_pyr_borders for it, direct above it)
    ((120, 160), 1.2, 8),    # frames wider than a wave's columns at the small levels, mirrored groups at every alignment
    ((150, 200), 1.2, 8),
    ((120, 264), 1.2, 8),    # level 1 is 220 wide: 65 groups, a second wave with one live lane
    ((480, 640), 1.2, 8),    # the benchmark's own levels
    ((376, 1241), 1.2, 8),   # four or more waves per row
    ((120, 160), 1.5, 4),    # 7-byte windows
    ((120, 160), 2.0, 3),    # 8-byte windows, every source row used, short strips
    ((120, 160), 1.1, 8),
    ((480, 640), 2.5, 3),    # 10-byte windows: the old kernel on every level
]


def _same(res_a, res_b, what):
    (n_a, k_a, d_a, m_a), (n_b, k_b, d_b, m_b) = res_a, res_b
    assert (n_a, m_a) == (n_b, m_b), what
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(k_a[f], k_b[f]), (what, f)
    assert np.array_equal(d_a, d_b), what


def _extractor(capi, switch, **kw):
    """A handle of its own: the switch is read once, when the handle is created."""
    old = os.environ.get("DVM_PYR_DIRECT")
    os.environ["DVM_PYR_DIRECT"] = switch
    try:
        return capi.OrbExtractor(max_batch=B, **kw)
    finally:
        if old is None:
            del os.environ["DVM_PYR_DIRECT"]
        else:
            os.environ["DVM_PYR_DIRECT"] = old


def _batch(shape, seed0):
    from dvm_slam_amd import synth
    imgs = np.stack([synth.small_image(seed0 + k, *shape) for k in range(B)])
    imgs[4] = 127
    return imgs


def _expected_paths(e, nlevels):
    """Which levels the direct kernel takes, from the handle's own level sizes and pitches."""
    dims = [e.pyramid(0, l)[1:] for l in range(nlevels)]   # (rows, cols, pitch)
    out = [0]
    for l in range(1, nlevels):
        (ph, pw, ps), (h, w, _) = dims[l - 1], dims[l]
        xofs = model.axis_tables(pw, w, True)[0]
        yofs = model.axis_tables(ph, h, False)[0]
        out.append(int(model.strip_rows(pw, ph, ps, w, h, xofs, yofs) > 0))
    return out


def _check_levels(e, orc, imgs, frames, nlevels, what):
    for f in frames:
        orc.extract(imgs[f])
        for l in range(nlevels):
            assert np.array_equal(e.debug_level(f, l, bordered=True), orc.level(l, bordered=True)), (what, f, l)


@pytest.mark.parametrize("shape,scale,nlevels", CASES)
def test_both_kernels_equal_each_other_and_the_oracle(capi, oracle, shape, scale, nlevels):
    imgs = _batch(shape, 40)
    orc = oracle.OrbOracle(scale_factor=scale, nlevels=nlevels)
    lv = {}
    for switch in ("1", "0"):
        e = _extractor(capi, switch, scale_factor=scale, nlevels=nlevels)
        e.extract_batch_host(imgs)
        paths = [e.debug_pyr_path(l) for l in range(nlevels)]
        want = _expected_paths(e, nlevels) if switch == "1" else [0] * nlevels
        assert paths == want, (switch, paths, want)
        if switch == "1":   # the case runs what it is meant to run
            if shape == (97, 131):
                assert paths == [0, 1, 1, 1, 1, 1, 1, 0]
            elif scale == 2.5:
                assert paths == [0, 0, 0]
            else:
                assert paths == [0] + [1] * (nlevels - 1)
        lv[switch] = {(f, l): e.debug_level(f, l, bordered=True) for f in (0, B - 1) for l in range(nlevels)}
        res8 = e.download(B - 1)
        e.close()
        ref8 = orc.extract(imgs[B - 1])
        _same(res8, ref8, (switch, "frame 8 vs oracle"))
        for l in range(nlevels):
            assert np.array_equal(lv[switch][(B - 1, l)], orc.level(l, bordered=True)), (switch, B - 1, l)
    orc.extract(imgs[0])
    for l in range(nlevels):
        assert np.array_equal(lv["1"][(0, l)], orc.level(l, bordered=True)), ("1", 0, l)
        for f in (0, B - 1):
            assert np.array_equal(lv["1"][(f, l)], lv["0"][(f, l)]), (f, l)


def test_path_switches_between_calls_on_one_handle(capi, oracle):
    """A second batch on the same handle, then a batch of one (the latency path's k_pyr_resize<16>), then a batch of nine again."""
    shape, L = (150, 200), 8
    orc = oracle.OrbOracle()
    e = _extractor(capi, "1")
    for seed0, nb in ((60, B), (80, B), (100, 1), (120, B)):
        imgs = _batch(shape, seed0)[:nb]
        e.extract_batch_host(imgs)
        assert [e.debug_pyr_path(l) for l in range(L)] == ([0] + [1] * (L - 1) if nb == B else [0] * L), (seed0, nb)
        _check_levels(e, orc, imgs, sorted({0, nb - 1}), L, (seed0, nb))   # (orc now holds the batch's last frame)
        _same(e.download(nb - 1), orc.extract(imgs[nb - 1]), (seed0, nb))
    e.close()
