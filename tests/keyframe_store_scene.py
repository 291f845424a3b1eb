"""TEST INFRASTRUCTURE for dvm_keyframe_store: random keyframes of a given size (a share of the keypoints outside the image bounds, so
that the grid holds fewer than n), the grid a slot must hold restated in numpy, and the comparison of a slot read back with the keyframe
that was put."""
import numpy as np

from oracle import pyoracle as po

L = 8
SF = (np.float32(1.2) ** np.arange(L)).astype(np.float32)
BOUNDS = np.array([0.0, 640.0, 0.0, 480.0], np.float32)
K = np.array([500.0, 501.0, 320.0, 240.0], np.float32)
GRID_COLS, GRID_ROWS = 64, 48


def keyframe(seed, n, fv=True, bounds=BOUNDS):
    """A keyframe dict as capi.KeyframeStore.put takes it: n keypoints (about 5 % outside the bounds), a FeatureVector over all of them."""
    rng = np.random.default_rng([seed, n, 911])
    kps = np.zeros(n, po.KP_DTYPE)
    kps["x"] = rng.uniform(bounds[0] - 20, bounds[1] + 20, n); kps["y"] = rng.uniform(bounds[2] - 15, bounds[3] + 15, n)
    kps["octave"] = rng.integers(0, L, n); kps["angle"] = rng.uniform(0, 360, n); kps["size"] = 31.0 * SF[kps["octave"]]
    kps["response"] = rng.uniform(0, 100, n); kps["class_id"] = -1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kf = dict(kps=kps, desc=desc, K=K + np.float32(seed % 7), bounds=np.asarray(bounds, np.float32), scale_factors=SF, level_sigma2=(SF * SF).astype(np.float32),
              inv_level_sigma2=(np.float32(1.0) / (SF * SF)).astype(np.float32), log_scale_factor=float(np.log(np.float32(1.2))))
    if fv and n:
        node = rng.integers(0, max(n // 6, 1), n) * 5 + 2
        if n >= 4:
            node[rng.integers(0, n)] = -1                        # the node that is last as unsigned
        order = np.argsort(node.astype(np.uint32), kind="stable")
        nodes, counts = np.unique(node.astype(np.uint32), return_counts=True)
        kf["fv"] = dict(fv_nodes=nodes.astype(np.int32), fv_off=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), fv_feat=order.astype(np.int32))
    return kf


def grid_of(kf):
    """(n_sorted, skp[n_sorted, 4] float32 bit patterns, sidx, sdesc, cell_start[64 * 48 + 1]) as frame_build_block leaves them: PosInGrid in
    float32 with round-half-away, keypoints outside the grid not indexed, order by (column, row, keypoint index)."""
    kps, b = kf["kps"], np.asarray(kf["bounds"], np.float32)
    w_inv = np.float32(GRID_COLS) / np.float32(b[1] - b[0]); h_inv = np.float32(GRID_ROWS) / np.float32(b[3] - b[2])

    def cell(v, lo, inv):
        f = ((v.astype(np.float32) - lo) * inv).astype(np.float64)
        return (np.sign(f) * np.floor(np.abs(f) + 0.5)).astype(np.int64)
    px, py = cell(kps["x"], b[0], w_inv), cell(kps["y"], b[2], h_inv)
    inside = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    idx = np.flatnonzero(inside)
    c = px[idx] * GRID_ROWS + py[idx]
    order = np.lexsort((idx, c))
    sidx, c = idx[order].astype(np.int32), c[order]
    skp = np.zeros((len(sidx), 4), np.float32)
    skp[:, 0] = kps["x"][sidx]; skp[:, 1] = kps["y"][sidx]
    skp.view(np.int32)[:, 2] = kps["octave"][sidx]; skp.view(np.int32)[:, 3] = c
    cell_start = np.searchsorted(c, np.arange(GRID_COLS * GRID_ROWS + 1), side="left").astype(np.int32)
    return len(sidx), skp, sidx, kf["desc"][sidx], cell_start


def assert_slot_is(r, kf):
    """r = KeyframeStore.read(slot); byte for byte the keyframe dict kf and its grid."""
    n = len(kf["kps"])
    fv = kf.get("fv")
    assert r["n"] == n and r["n_total"] == n and r["n_levels"] == len(kf["scale_factors"])
    assert r["kps"].tobytes() == np.ascontiguousarray(kf["kps"], po.KP_DTYPE).tobytes() and r["desc"].tobytes() == kf["desc"].tobytes()
    assert r["fv_n"] == (len(fv["fv_nodes"]) if fv else 0) and r["n_feat"] == (len(fv["fv_feat"]) if fv else 0)
    if fv:
        for k in ("fv_nodes", "fv_off", "fv_feat"):
            assert np.array_equal(r[k], fv[k]), k
    else:
        assert len(r["fv_off"]) == 0
    for k in ("scale_factors", "level_sigma2", "inv_level_sigma2"):
        assert r[k].tobytes() == np.asarray(kf[k], np.float32).tobytes(), k
    assert r["K"].tobytes() == np.asarray(kf["K"], np.float32).tobytes() and r["bounds"].tobytes() == np.asarray(kf["bounds"], np.float32).tobytes()
    assert np.float32(r["log_scale_factor"]) == np.float32(kf["log_scale_factor"])
    ns, skp, sidx, sdesc, cell_start = grid_of(kf)
    assert r["n_sorted"] == ns
    assert r["skp"].tobytes() == skp.tobytes() and np.array_equal(r["sidx"], sidx) and r["sdesc"].tobytes() == sdesc.tobytes()
    assert np.array_equal(r["cell_start"][:GRID_COLS * GRID_ROWS + 1], cell_start)
