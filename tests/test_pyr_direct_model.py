"""CPU model of k_pyr_resize_direct (tests/pyr_direct_model.py) against the oracle: bitwise, every level of every shape the GPU test
runs, plus the eligibility verdicts and the exhaustive check of the vertical pass's v_mul_hi_u32_u24 form."""
import numpy as np
import pytest

import pyr_direct_model as m

# (rows, cols), scale factor, levels
CASES = [((97, 131), 1.2, 8), ((120, 160), 1.2, 8), ((150, 200), 1.2, 8), ((120, 264), 1.2, 8), ((480, 640), 1.2, 8),
         ((376, 1241), 1.2, 8), ((480, 752), 1.2, 8), ((120, 160), 1.5, 4), ((120, 160), 2.0, 3), ((120, 160), 1.1, 8),
         ((480, 640), 1.1, 8)]


def _levels(oracle, shape, scale, nlevels, seed=7):
    from dvm_slam_amd import synth
    orc = oracle.OrbOracle(scale_factor=scale, nlevels=nlevels)
    orc.extract(synth.small_image(seed, *shape))
    return orc, [orc.level_dims(l) for l in range(nlevels)]


def _verdict(dims, l):
    (ph, pw), (h, w) = dims[l - 1], dims[l]
    xofs = m.axis_tables(pw, w, True)[0]
    yofs = m.axis_tables(ph, h, False)[0]
    return m.strip_rows(pw, ph, m.align_up(pw + 2 * m.EDGE, 64), w, h, xofs, yofs)


@pytest.mark.parametrize("shape,scale,nlevels", CASES)
def test_model_equals_the_oracle(oracle, shape, scale, nlevels):
    orc, dims = _levels(oracle, shape, scale, nlevels)
    direct = 0
    for l in range(1, nlevels):
        (ph, pw), (h, w) = dims[l - 1], dims[l]
        R = _verdict(dims, l)
        tiny = w < 40 or h < 20 or pw < 40 or ph < 20
        assert (R == 0) == tiny, (l, R)      # at these scales every level that is not tiny qualifies
        if R == 0:
            continue
        direct += 1
        pstride = m.align_up(pw + 2 * m.EDGE, 64)
        parent = np.full((ph + 2 * m.EDGE, pstride), 0x55, np.uint8)   # pad bytes of the pitch: never selected
        parent[:, :pw + 2 * m.EDGE] = orc.level(l - 1, bordered=True)
        got = m.resize_direct(parent, pw, ph, w, h, R)
        bw = w + 2 * m.EDGE
        assert np.array_equal(got[m.EDGE:m.EDGE + h, m.EDGE:m.EDGE + w], oracle.resize_linear(orc.level(l - 1), w, h)), l
        assert np.array_equal(got[:, :bw], orc.level(l, bordered=True)), l
        # pad bytes of the last group repeat the last frame column; nothing is written beyond that group
        end = m.align_up(bw, 4)
        assert (got[:, bw:end] == got[:, bw - 1:bw]).all() and (got[:, end:] == 0xCC).all(), l
    assert direct >= 2


def test_strip_heights():
    """R = 16 or more at scale 1.2 (strips of up to 24 source rows), every source row used at scale 2."""
    dims = [(480, 640), (400, 533), (333, 444)]
    assert _verdict(dims, 1) >= 16 and _verdict(dims, 2) >= 16
    assert _verdict([(120, 160), (60, 80)], 1) == m.NS // 2


def test_refused(oracle):
    _, dims = _levels(oracle, (480, 640), 2.5, 3)
    assert [_verdict(dims, l) for l in (1, 2)] == [0, 0]            # 10-byte windows
    _, dims = _levels(oracle, (97, 131), 1.2, 8)
    assert dims[7][1] < 40 and _verdict(dims, 7) == 0               # a tiny level
    assert all(_verdict(dims, l) > 0 for l in range(1, 7))
    dims = [(23, 100), (19, 83), (16, 69)]
    assert _verdict(dims, 1) == 0 and _verdict(dims, 2) == 0        # a tiny level, and the child of one
    # a level as large as its parent: the last row's second tap is clamped -> refused
    xofs = m.axis_tables(64, 64, True)[0]
    assert m.strip_rows(64, 48, 128, 64, 48, xofs, m.axis_tables(48, 48, False)[0]) == 0
    # upsampling repeats source rows -> refused
    assert m.strip_rows(64, 40, 128, 64, 48, xofs, m.axis_tables(40, 48, False)[0]) == 0


def test_mul_hi_identity_exhaustive():
    """(b << 12) * (h & ~15) >> 32 == (b * (h >> 4)) >> 16 for every weight b in [0, 2048] and every h >> 4 in [0, 32640]."""
    q = np.arange(0, 32641, dtype=np.uint64)
    assert int(q[-1]) << 4 < 1 << 24 and 2048 << 12 < 1 << 24
    for b in range(0, 2049):
        assert np.array_equal(m.mul_hi_u24(b << 12, q << np.uint64(4)), (np.uint64(b) * q) >> np.uint64(16)), b
