"""numpy restatement of k_pyr_resize_direct (dvm_slam_amd/csrc/orb_kernels.hip): the resize tables of OrbPipeline::configure, the
eligibility test pyr_direct_strip_rows(), and the kernel's index arithmetic -- window base, v_perm selectors, pad-column rule, the
strip's source-row walk with its emit test, the v_mul_hi_u32_u24 form of the vertical pass, strip-row mirroring.

Shared by tests/test_pyr_direct_model.py (CPU) and tests/test_gpu_pyr_direct.py (which level takes which kernel)."""
import numpy as np

EDGE = 19
NS = 24   # kRdNS: source rows of a strip


def align_up(x, a):
    return (x + a - 1) // a * a


def axis_tables(ssize, dsize, clamp_like_x):
    """resize_axis_tables(): cv::resize INTER_LINEAR offsets and (w0 | w1 << 16) 11-bit weights of one axis."""
    sc = 1.0 / (float(dsize) / float(ssize))
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * sc - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_like_x:
        lo, hi = s < 0, s >= ssize - 1
        f[lo] = 0
        s[lo] = 0
        f[hi] = 0
        s[hi] = ssize - 1
    w0 = np.rint((np.float32(1.0) - f) * np.float32(2048)).astype(np.int64)
    w1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, w0, w1


def group_columns(w):
    """Per 4-byte group of the bordered row (X4 = 0, 4, ...) the interior column each byte takes its value from: REFLECT_101 for
    frame columns, the last frame column again for pad bytes beyond the frame."""
    bw = w + 2 * EDGE
    X = np.arange(0, align_up(bw, 4)).reshape(-1, 4)
    x = np.minimum(X, bw - 1) - EDGE
    return np.where(x < 0, -x, np.where(x >= w, 2 * (w - 1) - x, x))


def strip_rows(pw, ph, pstride, w, h, xofs, yofs, ns=NS):
    """pyr_direct_strip_rows(): the strip height R of the direct kernel for a level, 0 = the level keeps k_pyr_resize."""
    if w < 40 or h < 20 or pw < 40 or ph < 20:
        return 0
    xm = group_columns(w)
    if xm.min() < 0 or xm.max() >= w:
        return 0
    lo, hi = xofs[xm].min(axis=1), xofs[xm].max(axis=1) + 1
    if (lo < 0).any() or (hi - lo + 1 > 8).any() or (EDGE + lo + 8 > pstride).any():
        return 0
    if (yofs < 0).any() or (yofs + 1 > ph - 1).any() or (np.diff(yofs) <= 0).any():   # no clamped tap, one emit per source row
        return 0
    r0, r1 = yofs, yofs + 1
    for R in range(min(ns, 63), 0, -1):
        y0 = np.arange(0, h, R)
        if (r1[np.minimum(y0 + R - 1, h - 1)] - r0[y0] + 1 <= ns).all():
            return R
    return 0


def mul_hi_u24(a, b):
    a, b = np.asarray(a, np.uint64) & np.uint64(0xFFFFFF), np.asarray(b, np.uint64) & np.uint64(0xFFFFFF)
    return (a * b) >> np.uint64(32)


def mirror_rows(y, h):
    top = EDGE - y if 1 <= y <= EDGE else -1
    bot = 2 * h + EDGE - 2 - y if h - 1 - EDGE <= y <= h - 2 else -1
    return top, bot


def resize_direct(parent, pw, ph, w, h, R, ns=NS, fill=0xCC):
    """The bytes k_pyr_resize_direct writes for one level.  parent: the parent's bordered buffer, (ph + 38) x pitch with pitch a
    multiple of 64 (only rows 19 .. ph + 18 are read).  Returns the (h + 38) x pitch destination buffer, `fill` where nothing is written."""
    pstride = parent.shape[1]
    stride = align_up(w + 2 * EDGE, 64)
    bw = w + 2 * EDGE
    xofs, xa0, xa1 = axis_tables(pw, w, True)
    yofs, yb0, yb1 = axis_tables(ph, h, False)
    flat = parent.reshape(-1)
    out = np.full((h + 2 * EDGE, stride), fill, np.uint8)
    ngroups = -(-bw // 4)
    for wave0 in range(0, ngroups, 64):
        lanes = np.arange(wave0, wave0 + 64)
        live = lanes * 4 < bw
        X4 = np.where(live, lanes * 4, (bw - 1) & ~3)
        xm = group_columns(w)[X4 // 4]                      # (64, 4)
        sx, a0, a1 = xofs[xm], xa0[xm], xa1[xm]
        base = sx.min(axis=1)
        i0, i1 = sx - base[:, None], sx + 1 - base[:, None]  # selector bytes
        assert i1.max() <= 7 and (EDGE + base + 8 <= pstride).all()
        for y0 in range(0, h, R):
            yl = min(y0 + R - 1, h - 1)
            sya, syb = int(yofs[y0]), int(yofs[yl]) + 1
            assert 0 <= sya and syb <= ph - 1
            assert syb - sya + 1 <= ns
            d = y0
            prev = None
            for j in range(ns):
                if sya + j > syb:
                    break
                at = (EDGE + sya + j) * pstride + EDGE + base
                win = flat[at[:, None] + np.arange(8)].astype(np.int64)   # the unaligned 8-byte load
                s0 = np.take_along_axis(win, i0, axis=1)
                s1 = np.take_along_axis(win, i1, axis=1)
                cur = (s0 * a0 + s1 * a1) & 0xFFFFF0
                if d <= yl and int(yofs[d]) + 1 == sya + j:
                    assert prev is not None
                    t0 = prev
                    b0, b1 = int(yb0[d]) << 12, int(yb1[d]) << 12
                    r = (mul_hi_u24(b0, t0) + mul_hi_u24(b1, cur) + np.uint64(2)) >> np.uint64(2)
                    assert r.max() <= 255
                    r = r.astype(np.uint8)
                    top, bot = mirror_rows(d, h)
                    nl = int(live.sum())   # (the live lanes are the first nl of the wave, their groups consecutive)
                    for row in (EDGE + d, top, bot):
                        if row >= 0:
                            out[row, X4[0]:X4[0] + 4 * nl] = r[:nl].reshape(-1)
                    d += 1
                prev = cur
            assert d == yl + 1   # every row of the strip was emitted
    return out
