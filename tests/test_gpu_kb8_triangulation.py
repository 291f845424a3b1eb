"""dvm_triangulate_matches_cam and dvm_match_triangulation_cam on KannalaBrandt8 keyframes against the float64 statements of
tests/kb8_tri_scene.py (pinned on the CPU by tests/test_kb8_tri_model.py): decisions where the margin exceeds 2e-3, x3D within the measured
allowance.  Pair counts around the geometry block of 128 threads, candidate lists around the row of 16 lanes."""
import functools

import numpy as np
import pytest

import kb8_scene as ks
import kb8_tri_scene as kt
import tri_scene

pytestmark = pytest.mark.gpu


def _cam(capi, p):
    return capi.CameraModel.make(capi.CameraModel.KANNALA_BRANDT8, p)


def _tri(capi, S, **kw):
    return capi.triangulate_matches_cam(_cam(capi, S["cam1"]), _cam(capi, S["cam2"]), S["T1w"], S["T2w"], S["Ow1"], S["Ow2"], S["kps1"], S["kps2"], S["pairs"],
                                        S["sigma2_1"], S["sigma2_2"], S["sf1"], S["sf2"], S["ratio_factor"], **kw)


def _compare(X, st, ref, what, n_small=False):
    Xr, sr, mg = ref
    clear = mg > kt.MARGIN
    print(f"{what}: left out {(~clear).mean():.4f}")
    if len(sr) >= 100:
        assert (~clear).mean() <= kt.LEFT_OUT_MAX
    assert np.array_equal(st[clear], sr[clear]), what
    tri = clear & (sr != 1) & (sr != -1)
    if tri.any():
        rel = np.linalg.norm(X[tri] - Xr[tri], axis=1) / np.linalg.norm(Xr[tri], axis=1)
        amax, amed = kt.x3d_allowance()
        print(f"    x3D relative difference, largest {rel.max():.3g} (allowed {amax:.3g}), median {np.median(rel):.3g} (allowed {amed:.3g})")
        assert rel.max() < amax
        if tri.sum() >= 20:
            assert np.median(rel) < amed
    assert np.all(X[(st == 1) | (st == -1)] == 0)


@pytest.mark.parametrize("n", [1, 127, 128, 129, 700])
@pytest.mark.parametrize("model", list(ks.MODELS))
def test_triangulate_matches_cam(capi, model, n):
    S = kt.scene(model, 20 + n % 7, n, 0.6)
    X, st = _tri(capi, S)
    _compare(X, st, kt.pair_geometry_ref(S), f"{model} n={n}")
    if n >= 127:
        assert {0, 1, 5, 6} <= set(np.unique(st).tolist())


def test_other_camera_pyramid_inertial_gate_and_far_points(capi):
    S = kt.scene("tum", 31, 700, 0.6, other=True)
    for kw in (dict(), dict(cos_parallax_max=0.9996), dict(far_points=True, th_far=7.5)):
        X, st = _tri(capi, S, **kw)
        _compare(X, st, kt.pair_geometry_ref(S, **kw), str(kw))
    assert (st == 8).sum() > 10
    # a short baseline: many rays are too parallel
    S = kt.scene("robomaster", 32, 700, 0.05)
    X, st = _tri(capi, S)
    _compare(X, st, kt.pair_geometry_ref(S), "baseline 0.05")
    assert (st == 1).sum() > 700 // 3


def test_octave_outside_the_tables_and_bad_arguments(capi):
    S = dict(kt.scene("robomaster", 33, 129, 0.6))
    k = S["kps1"].copy(); k["octave"][S["pairs"][0, 0]] = 9
    k2 = S["kps2"].copy(); k2["octave"][S["pairs"][5, 1]] = -1
    S["kps1"], S["kps2"] = k, k2
    X, st = _tri(capi, S)
    assert st[0] == -1 and st[5] == -1 and np.all(X[0] == 0) and np.all(X[5] == 0)
    _compare(X, st, kt.pair_geometry_ref(S), "octaves outside")
    bad = S["pairs"].copy(); bad[3, 1] = len(S["kps2"])
    with pytest.raises(capi.DvmError):
        _tri(capi, dict(S, pairs=bad))
    X, st = _tri(capi, dict(S, pairs=np.zeros((0, 2), np.int32)))
    assert X.shape == (0, 3) and st.shape == (0,)


def test_model_0_is_the_pinhole_entry(capi):
    S = tri_scene.scene(seed=9, n=700, K2=(430.0, 431.0, 350.0, 240.0))
    args = (S["T1w"], S["T2w"], S["Ow1"], S["Ow2"], S["kps1"], S["kps2"], S["pairs"], S["sigma2_1"], S["sigma2_2"], S["sf1"], S["sf2"], S["ratio_factor"])
    for kw in (dict(), dict(far_points=True, th_far=7.5)):
        Xp, sp = capi.triangulate_matches(S["K1"], S["K2"], *args, **kw)
        Xc, sc = capi.triangulate_matches_cam(capi.CameraModel.pinhole(*S["K1"]), capi.CameraModel.pinhole(*S["K2"]), *args, **kw)
        assert np.array_equal(sp, sc) and np.array_equal(Xp.view(np.uint32), Xc.view(np.uint32))
    assert (sp == 0).sum() > 100


def _search(capi, SS, coarse=False):
    return capi.match_triangulation_cam(SS["desc1"], SS["kps1"], SS["qidx"], SS["desc2"], SS["kps2"], SS["off"], SS["cand"], _cam(capi, SS["cam1"]),
                                        _cam(capi, SS["cam2"]), capi.pair_pose(SS["R12"], SS["t12"]), SS["ep"], coarse, SS["sigma2_1"], SS["sf2"], SS["sigma2_2"])


@functools.lru_cache(maxsize=None)
def _search_ref(model, nq, coarse):
    return kt.search_ref(kt.search_scene(model, 0, nq, other=(model == "tum")), coarse)


@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("nq", [1, 15, 16, 17, 257])
@pytest.mark.parametrize("model", list(ks.MODELS))
def test_match_triangulation_cam(capi, model, nq, coarse):
    """Lists of 0, 1, 15, 16, 17 and 33 candidates; ties go to the last candidate; coarse skips the constraint."""
    SS = kt.search_scene(model, 0, nq, other=(model == "tum"))
    bi, bd = _search(capi, SS, coarse)
    ri, rd, cmp_ = _search_ref(model, nq, coarse)
    print(f"{model} nq={nq} coarse={coarse}: left out {(~cmp_).mean():.4f}, found {(ri >= 0).sum()}")
    assert (~cmp_).mean() <= kt.LEFT_OUT_MAX
    assert np.array_equal(bi[cmp_], ri[cmp_]) and np.array_equal(bd[cmp_], rd[cmp_])
    assert np.all(bd[bi < 0] == 256)
    if nq == 257:
        assert (bi >= 0).sum() > 100
        if not coarse:
            assert (bi != _search_ref(model, nq, True)[0]).sum() > 40          # the constraint decided something


def test_match_triangulation_cam_octaves_outside_the_tables(capi):
    """A query whose octave lies outside KF1's table finds nothing (coarse: it is matched, KF1's table is not read); a candidate whose
    octave lies outside KF2's tables is no candidate."""
    SS = dict(kt.search_scene("robomaster", 0, 257))
    ri, _, cmp_ = kt.search_ref(SS)
    found = np.nonzero((ri >= 0) & cmp_)[0]
    qa, qb = int(found[0]), int(found[1])
    k1 = SS["kps1"].copy(); k1["octave"][qa] = 8
    k2 = SS["kps2"].copy(); k2["octave"][ri[qb]] = -1
    bi, bd = _search(capi, dict(SS, kps1=k1, kps2=k2))
    assert bi[qa] == -1 and bd[qa] == 256 and bi[qb] != ri[qb]
    keep = cmp_ & (np.arange(257) != qa) & (ri != ri[qb])
    assert np.array_equal(bi[keep], ri[keep])
    bi, _ = _search(capi, dict(SS, kps1=k1), coarse=True)
    assert bi[qa] >= 0


def test_more_survivors_than_the_workgroup_list_holds(capi):
    """16 queries whose 33 candidates are all the true match: 528 candidates pass the distance and disc tests in one workgroup, more than
    its list of 256 holds, so the rest go through the constraint where they stand; every tie still goes to the last position."""
    SS = dict(kt.search_scene("robomaster", 0, 16))
    SS["cand"] = np.repeat(np.arange(16, dtype=np.int32), 33); SS["off"] = (np.arange(17) * 33).astype(np.int32)
    ri, rd, cmp_ = kt.search_ref(SS)
    assert cmp_.sum() >= 12 and (ri[cmp_] >= 0).sum() >= 8
    bi, bd = _search(capi, SS)
    assert np.array_equal(bi[cmp_], ri[cmp_]) and np.array_equal(bd[cmp_], rd[cmp_])
