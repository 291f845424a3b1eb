"""dvm_fuse_targets_set_cam: the Fuse chain with a camera model and a form per target.  Pinhole targets in the Scw form against the
oracle's ungated rows; KannalaBrandt8 targets bit for bit against the loop of dvm_project_search_cam they batch (same device function, so no
margin) and against kb8_scene's numpy restatement on the pairs its margin rule keeps; mixed calls row by row against their single calls.
Integers are compared exactly.  The scenes are pinned by tests/test_fuse_cam_scene.py (CPU)."""
import ctypes as C
import functools

import numpy as np
import pytest

import fuse_cam_scene as fcs
import fuse_targets_scene as fts
import kb8_scene as ks

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 200]             # 16-lane rows, 16 rows per block
KB8_SIZES = [1, 15, 16, 17, 900]


@pytest.fixture(scope="module")
def chain(capi):
    h = capi.FuseTargets()
    h.reserve(900, 33, 33 * 300 + 2000)
    yield h
    h.close()


def _prefix(pts, n):
    return {k: v[:n].copy() for k, v in pts.items()}


def _chain_pts(pts, use_valid):
    return {k: v for k, v in pts.items() if k in ("pos", "normal", "min_dist", "max_dist", "desc") or (use_valid and k == "valid")}


@functools.lru_cache(maxsize=None)
def _scw_oracle(T, n, masked, gate=False):
    sc = fcs.scw_scene(T)
    pts = _prefix(sc["pts"], n)
    skip = ((sc["skip"][:, :n] != 0) | (pts["valid"][None, :] == 0)).astype(np.uint8) if masked else None
    return fcs.scw_rows(sc["targets"], pts, skip, gate=gate)


@pytest.mark.parametrize("masked", [False, True], ids=("plain", "masked_valid"))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("T", [1, 2, 5, 33])
def test_scw_form_against_the_ungated_oracle(chain, T, n, masked):
    sc = fcs.scw_scene(T)
    pts = _prefix(sc["pts"], n)
    chain.set([fcs.chain_target(kf) for kf in sc["targets"]], forms=[chain.FORM_SCW] * T)
    bi, bd = chain.run(_chain_pts(pts, masked), fcs.TH, sc["skip"][:, :n] if masked else None)
    want_i, want_d = _scw_oracle(T, n, masked)
    assert np.array_equal(bi, want_i) and np.array_equal(bd, want_d)
    if n == 200 and not masked:
        gated = _scw_oracle(T, n, masked, gate=True)
        assert (want_i != gated[0]).sum() >= 5                                          # the form matters on this scene
    # inv_level_sigma2 is not read in this form and may be missing
    chain.set([dict(fcs.chain_target(kf), inv_level_sigma2=None, level_sigma2=None) for kf in sc["targets"]], forms=[chain.FORM_SCW] * T)
    bi2, bd2 = chain.run(_chain_pts(pts, masked), fcs.TH, sc["skip"][:, :n] if masked else None)
    assert np.array_equal(bi2, want_i) and np.array_equal(bd2, want_d)


def test_mixed_forms_row_by_row(chain):
    T = 33
    sc = fcs.scw_scene(T)
    tg = [fcs.chain_target(kf) for kf in sc["targets"]]
    pts = _chain_pts(sc["pts"], True)
    rows = {}
    for f in (0, 1):
        chain.set(tg, forms=[f] * T)
        rows[f] = chain.run(pts, fcs.TH, sc["skip"])
    forms = np.arange(T) % 2
    chain.set(tg, forms=forms)
    bi, bd = chain.run(pts, fcs.TH, sc["skip"])
    for t in range(T):
        assert np.array_equal(bi[t], rows[forms[t]][0][t]) and np.array_equal(bd[t], rows[forms[t]][1][t]), t
    assert sum((rows[0][0][t] != rows[1][0][t]).any() for t in range(T)) >= 10           # the two forms differ on many rows
    want = _scw_oracle(T, 200, True), _scw_oracle(T, 200, True, gate=True)
    assert np.array_equal(rows[1][0], want[0][0]) and np.array_equal(rows[0][0], want[1][0])


@pytest.mark.parametrize("T", [1, 2, 5, 33])
def test_null_models_and_pinhole_models_are_set(capi, chain, T):
    """set_cam(NULL, NULL) and model-0 structs on every target (their p[0..3] replace the targets' own intrinsics, which are then not
    read): byte-equal to set + run."""
    sc = fts.prefix(fts.scene(fcs.SEED_OF_T[T], T), 200)
    chain.set(sc["targets"])
    a = chain.run(sc["pts"], 3.0, sc["skip"])
    chain.set(sc["targets"], forms=[0] * T)                                              # (models NULL)
    b = chain.run(sc["pts"], 3.0, sc["skip"])
    arr, keep = chain.targets(sc["targets"])
    capi.check(chain.L.dvm_fuse_targets_set_cam(chain.h, T, C.addressof(arr), None, None))
    c = chain.run(sc["pts"], 3.0, sc["skip"])
    models = [capi.CameraModel.pinhole(*kf["K"]) for kf in sc["targets"]]
    chain.set([dict(kf, K=np.array([9.0, 9.0, 9.0, 9.0], np.float32)) for kf in sc["targets"]], models=models)
    d = chain.run(sc["pts"], 3.0, sc["skip"])
    for x in (b, c, d):
        assert x[0].tobytes() == a[0].tobytes() and x[1].tobytes() == a[1].tobytes()
    assert (a[0] >= 0).sum() >= 0.1 * T * 200


# ---------------------------------------------------------------------------------------------------------------- KannalaBrandt8
def _model(capi, name):
    return capi.CameraModel.make(1, ks.MODELS[name])


def _single_call(capi, tg, model, pts, form, valid, th=fcs.KB8_TH):
    """dvm_project_search_cam on one target alone (tg: the keyframe dict the chain takes), then the `<= 50` rule: (best_idx, best_dist)."""
    n = len(pts["pos"])
    if len(tg["kps"]) == 0:
        return np.full(n, -1, np.int32), np.full(n, 256, np.int32)
    g = capi.FrameGrid(2048)
    g.build(tg["kps"], tg["desc"], tuple(float(v) for v in tg["bounds"]))
    cam = dict(Tcw=tg["Tcw"], Ow=tg["Ow"], bounds=tg["bounds"], log_scale_factor=tg["log_scale_factor"])
    m, _ = capi.project_search_cam(g, cam, model, pts, th, tg["scale_factors"], gate_inv_sigma2=tg["inv_level_sigma2"] if form == 0 else None, gate=5.99,
                                   valid=valid)
    g.close()
    return np.where(m["best_dist"] <= 50, m["best_idx"], -1).astype(np.int32), m["best_dist"].astype(np.int32)


@functools.lru_cache(maxsize=None)
def _kb8_ref(model, T, n, form):
    return fcs.kb8_rows(fcs.kb8_scene(model, T, n), form)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n", KB8_SIZES)
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("model", list(ks.MODELS))
def test_kb8_chain_is_the_loop_of_project_search_cam(capi, chain, model, T, n, form):
    sc = fcs.kb8_scene(model, T, n)
    pts = sc["pts"]
    mdl = _model(capi, model)
    chain.set([fcs.kb8_chain_target(tg) for tg in sc["targets"]], models=[mdl] * T, forms=[form] * T)
    ref_i, ref_d, drop = _kb8_ref(model, T, n, form)
    for masked in (False, True):
        bi, bd = chain.run(_chain_pts(pts, masked), fcs.KB8_TH, sc["skip"] if masked else None)
        valid = (1 - fcs.kb8_mask(sc, True)).astype(np.uint8) if masked else np.ones((T, n), np.uint8)
        for t, tg in enumerate(sc["targets"]):
            want_i, want_d = _single_call(capi, fcs.kb8_chain_target(tg), mdl, _chain_pts(pts, False), form, valid[t])
            assert np.array_equal(bi[t], want_i) and np.array_equal(bd[t], want_d), (t, masked)     # bit for bit: one device function
        # ... and the numpy restatement on the pairs its margin rule keeps
        keep = ~drop
        assert keep.sum() >= (1 - ks.DROP_MAX) * T * n
        wi = np.where(valid != 0, ref_i, -1); wd = np.where(valid != 0, ref_d, 256)
        assert np.array_equal(bi[keep], wi[keep]) and np.array_equal(bd[keep], wd[keep]), masked
    if n == 900:
        filled = [t for t in range(T) if len(sc["targets"][t]["kps"])]
        assert all((bi[t] >= 0).mean() >= 0.15 * 0.6 for t in filled)


@pytest.mark.parametrize("model", list(ks.MODELS))
def test_a_pinhole_and_a_kb8_target_in_one_call(capi, chain, model):
    """Rows are independent: each row of the mixed call equals its single call, whichever order the targets come in.  The point table is a
    fisheye cloud followed by the pinhole scene's, so that both targets find their own points."""
    ksc, psc = fcs.kb8_scene(model, 5, 600), fts.prefix(fts.scene(0, 5), 200)
    pts = {k: np.concatenate([ksc["pts"][k], psc["pts"][k]]) for k in ("pos", "normal", "min_dist", "max_dist", "desc", "valid")}
    pkf = psc["targets"][0]
    tg_k, tg_p = fcs.kb8_chain_target(ksc["targets"][0]), dict(pkf, Ow=capi.se3_inverse(pkf["Tcw"])[4:], K=np.full(4, 9.0, np.float32))
    kb8, pin = _model(capi, model), capi.CameraModel.pinhole(*pkf["K"])
    for order, forms in (((0, 1), [0, 1]), ((1, 0), [0, 0]), ((1, 0), [1, 0])):
        tg = [(tg_k, tg_p)[o] for o in order]
        models = [(kb8, pin)[o] for o in order]
        chain.set(tg, models=models, forms=forms)
        bi, bd = chain.run(pts, fcs.KB8_TH)
        for t in range(2):
            want_i, want_d = _single_call(capi, tg[t], models[t], _chain_pts(pts, False), forms[t], pts["valid"])
            assert np.array_equal(bi[t], want_i) and np.array_equal(bd[t], want_d), (t, forms)
            own = slice(0, 600) if order[t] == 0 else slice(600, 800)
            assert (bi[t][own] >= 0).sum() > 30, (t, forms)
    # the model decides the row: the same target under the other model answers otherwise
    chain.set([tg_k], models=[kb8]); a = chain.run(pts, fcs.KB8_TH)[1]
    chain.set([tg_k], models=[capi.CameraModel.pinhole(*ks.MODELS[model][:4])]); b = chain.run(pts, fcs.KB8_TH)[1]
    assert (a != b).mean() > 0.2


def test_host_entry_on_camera_models(capi, chain):
    sc = fts.prefix(fts.scene(0, 5), 200)
    P = capi.map_points_view(dict(sc["pts"], id=np.arange(200, dtype=np.int32), bad=1 - sc["pts"]["valid"]))
    views = [capi.keyframe_view(kf) for kf in sc["targets"]]
    n0, r0 = capi.fuse_targets(views, P, sc["skip"], 3.0)
    n1, r1 = capi.fuse_targets_cam(views, None, P, sc["skip"], 3.0)                      # models = None: fuse_targets
    assert n0 == n1 > 100 and r0.tobytes() == r1.tobytes()
    n2, r2 = capi.fuse_targets_cam(views, [capi.CameraModel.pinhole(*kf["K"]) for kf in sc["targets"]], P, sc["skip"], 3.0)
    assert n2 == n0 and r2.tobytes() == r0.tobytes()
    for model in ks.MODELS:
        ksc = fcs.kb8_scene(model, 5, 900)
        tg = [fcs.kb8_chain_target(x) for x in ksc["targets"]]
        mdl = [_model(capi, model)] * 5
        chain.set(tg, models=mdl)
        bi, _ = chain.run(_chain_pts(ksc["pts"], True), fcs.KB8_TH, ksc["skip"])
        KP = capi.map_points_view(dict(_chain_pts(ksc["pts"], False), bad=1 - ksc["pts"]["valid"]))
        n3, r3 = capi.fuse_targets_cam([capi.keyframe_view(x) for x in tg], mdl, KP, ksc["skip"], fcs.KB8_TH)
        assert np.array_equal(r3, bi) and n3 == (bi >= 0).sum() > 0.1 * 5 * 900
    with pytest.raises(capi.DvmError) as e:
        capi.fuse_targets_cam(views, [capi.CameraModel.make(2, [1, 1, 0, 0])] * 5, P, sc["skip"], 3.0)
    assert e.value.code == -1


def test_refusals_leave_the_handle_usable(capi):
    h = capi.FuseTargets()
    sc = fts.prefix(fts.scene(0, 5), 200)
    want = fts.oracle_rows(sc["targets"], sc["pts"], sc["skip"])
    h.reserve(200, 5, 5 * 300 + 2000)
    h.set(sc["targets"])
    pin = [capi.CameraModel.pinhole(*kf["K"]) for kf in sc["targets"]]

    def refused(what, fn):
        with pytest.raises(capi.DvmError) as e:
            fn()
        assert e.value.code == -1 and what in str(e.value), str(e.value)
        i, d = h.run(sc["pts"], 3.0, sc["skip"])                                      # ... the resident targets still serve
        assert np.array_equal(i, want[0]) and np.array_equal(d, want[1])
        h.set(sc["targets"], models=pin, forms=[0] * 5)                               # ... and so does a good set
        assert np.array_equal(h.run(sc["pts"], 3.0, sc["skip"])[0], want[0])

    def models(t, m):
        x = list(pin); x[t] = m
        return x
    refused("target 3", lambda: h.set(sc["targets"], models=models(3, capi.CameraModel.make(2, [500, 500, 320, 240]))))     # a model outside {0, 1}
    refused("target 1", lambda: h.set(sc["targets"], models=models(1, capi.CameraModel.make(-1, [500, 500, 320, 240]))))
    refused("target 2", lambda: h.set(sc["targets"], models=models(2, capi.CameraModel.make(1, [0, 500, 320, 240]))))       # zero focal length of a model
    refused("target 4", lambda: h.set(sc["targets"], models=models(4, capi.CameraModel.make(0, [500, 0, 320, 240]))))
    refused("target 0", lambda: h.set(sc["targets"], forms=[2, 0, 0, 0, 0]))                                                # a form outside {0, 1}
    refused("target 4", lambda: h.set(sc["targets"], models=pin, forms=[0, 1, 0, 1, 255]))
    # what the plain set refuses stays refused in both forms; a missing inv_level_sigma2 only in the gated form
    tg = list(sc["targets"]); tg[2] = dict(tg[2], inv_level_sigma2=None)
    refused("target 2", lambda: h.set(tg, forms=[1, 1, 0, 1, 1]))
    tg = list(sc["targets"]); tg[3] = dict(tg[3], K=np.array([0.0, 500.0, 320.0, 240.0], np.float32))
    refused("target 3", lambda: h.set(tg, forms=[1] * 5))                                                                   # its own focal length, no model given
    h.set(tg, models=pin, forms=[0] * 5)                                                                                    # ... which a model replaces
    assert np.array_equal(h.run(sc["pts"], 3.0, sc["skip"])[0], want[0])
    h.close()
