"""tests/map_refresh_scene.py on the CPU: the restatement's winner and median against the oracle's ComputeDistinctiveDescriptors and
against the definition written out with sorted rows; its float32 geometry against a float64 evaluation of the same inputs."""
import numpy as np
import pytest

import map_refresh_scene as S
from oracle import pyoracle as po

EPS = 2.0 ** -24          # float32 unit roundoff (round to nearest)


def _rows(rng, N, kind):
    if kind == "same":
        return np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), N, axis=0)
    if kind == "near":                                   # a few bits apart: many equal medians
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        rows = np.repeat(base[None], N, axis=0)
        for i in range(N):
            rows[i, rng.integers(0, 32)] ^= np.uint8(1 << rng.integers(0, 8))
        return rows
    return rng.integers(0, 256, (N, 32), dtype=np.uint8)


def _brute(rows):
    """the definition: per row the sorted list of its N distances (self included), its entry (N - 1) >> 1; first strictly smaller wins"""
    N = len(rows)
    best, best_med = -1, 1 << 30
    for i in range(N):
        dist = sorted(int(np.unpackbits(rows[i] ^ rows[j]).sum()) for j in range(N))
        m = dist[(N - 1) >> 1]
        if m < best_med:
            best, best_med = i, m
    return best, best_med


@pytest.mark.parametrize("kind", ["random", "near", "same"])
def test_winner_and_median(kind):
    rng = np.random.default_rng([39, len(kind)])
    sizes = [1, 2, 3, 4, 5, 17, 63, 64, 65, 130]
    rows = [_rows(rng, N, kind) for N in sizes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    bi, bm = po.distinctive_descriptors(np.concatenate(rows), off)
    for k, r in enumerate(rows):
        w, m = S.distinctive(r)
        assert (w, m) == (int(bi[k]), int(bm[k])), (kind, sizes[k])
        if sizes[k] <= 65:
            assert (w, m) == _brute(r), (kind, sizes[k])
    assert S.distinctive(np.zeros((0, 32), np.uint8)) == (-1, -1)


def test_hamming_table():
    rng = np.random.default_rng(5)
    r = rng.integers(0, 256, (9, 32), dtype=np.uint8)
    D = S.hamming_table(r)
    for i in range(9):
        for j in range(9):
            assert D[i, j] == np.unpackbits(r[i] ^ r[j]).sum()


@pytest.mark.parametrize("N", [1, 2, 3, 64, 65, 512])
def test_geometry_against_float64(N):
    """Tolerances from float32 rounding, eps = 2^-24, every input an exact float32:
      a term t = d / |d|: d one rounding (eps), |d| = sqrt(a0 + (a1 + a2)) of rounded squares at most 3.5 eps relative, the quotient one
        more -- |t_c| <= 1 is off by at most 6 eps;
      the sum of N terms one after another: partial sum i is at most i in size, so its rounding adds at most i eps -- N (N + 1) / 2 eps in
        all -- on top of the terms' 6 N eps; the division by N scales both by 1 / N and rounds once (|normal_c| <= 1):
        |normal_c - exact| <= (6 + (N + 1) / 2 + 1) eps;
      max_dist = |d| * sf: 3.5 eps + one rounding, bounded by 6 eps relative; min_dist = max_dist / sf_last: one more, 7 eps relative."""
    rng = np.random.default_rng([N, 3])
    sf = S.TABLES_B["scale_factors"]
    for trial in range(8):
        pos = (rng.uniform(-6, 6, 3) + [0, 0, 9]).astype(np.float32)
        ow = rng.uniform(-2, 2, (N, 3)).astype(np.float32)
        ref, octave = int(rng.integers(0, N)), int(rng.integers(0, len(sf)))
        g = S.geometry(pos, ow, ow[ref], sf, octave)
        assert g.dtype == np.float32 and np.array_equal(g[:3], pos)
        d = pos.astype(np.float64) - ow.astype(np.float64)
        exact = (d / np.linalg.norm(d, axis=1, keepdims=True)).sum(axis=0) / N
        assert np.abs(g[3:6].astype(np.float64) - exact).max() <= (7 + (N + 1) / 2) * EPS
        mx = np.linalg.norm(d[ref]) * np.float64(sf[octave])
        assert abs(float(g[7]) - mx) <= 6 * EPS * mx
        mn = mx / np.float64(sf[-1])
        assert abs(float(g[6]) - mn) <= 7 * EPS * mn


def test_refresh_ref_rules():
    """what the restatement writes: n_obs always; an old point keeps pos and bad; what selects the groups; a bad keyframe leaves the
    candidates but not the normal; a new point's record is whole with bad = 0"""
    kfs = [S.make_keyframe(k, 40 + k, S.TABLES_B if k % 2 else S.TABLES_A) for k in range(6)]
    sc = S.make_scene(1, kfs, [0, 1, 2, 5, 6, 6], bad=[1, 2], gone=[2], new=[4])
    before = sc["records"]
    rec, best, med, geo = S.refresh_ref(sc)
    assert np.array_equal(rec["n_obs"], [0, 1, 2, 5, 6, 6])
    assert rec[0].tobytes()[:64] == before[0].tobytes()[:64] and best[0] == -1
    old = sc["is_new"] == 0
    assert np.array_equal(rec["pos"][old], before["pos"][old]) and np.array_equal(rec["bad"][old], before["bad"][old])
    assert np.array_equal(rec["pos"][4], sc["new_pos"][4]) and rec["bad"][4] == 0
    for p in range(1, 6):
        o = sc["obs"][sc["obs_off"][p]:sc["obs_off"][p + 1]]
        if best[p] >= 0:
            assert not sc["bad"][o["kf"][best[p]]]
            assert np.array_equal(rec["desc"][p], kfs[o["kf"][best[p]]]["desc"][o["kp"][best[p]]])
    d_only = S.refresh_ref(sc, S.DESCRIPTOR)[0]
    g_only, b_g, _, _ = S.refresh_ref(sc, S.GEOMETRY)
    assert np.array_equal(d_only["normal"][old], before["normal"][old]) and np.array_equal(d_only["desc"], rec["desc"])
    assert np.array_equal(g_only["desc"][old], before["desc"][old]) and np.array_equal(g_only["normal"], rec["normal"]) and (b_g == -1).all()
    assert np.array_equal(geo[:, 3:6], rec["normal"]) and np.array_equal(geo[:, 7], rec["max_dist"])
