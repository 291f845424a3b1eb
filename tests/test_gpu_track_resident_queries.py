"""k_track_queries alone (dvm_track_debug_build_queries): the projection queries of the resident first half, built on the device from
LastFrame's entry lists and a map-point store, against the host's loop header (dvmh_build_frame_queries) bit for bit under the pinhole
camera: every array and nq, at the wave and round tails of the ordered compaction, with all entries kept, none kept and a mix in which
about a fifth fails each gate.  No images."""
import numpy as np
import pytest

import resident_scene as rs

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]


@pytest.fixture(scope="module")
def rig():
    from dvm_slam_amd import capi
    ext = capi.OrbExtractor(max_batch=3)
    trk = capi.TrackerBatch(ext, 3)
    yield capi, trk
    trk.close(); ext.close()


def _store(capi, e):
    st = capi.MapStore(len(e["records"]))
    st.update(np.arange(len(e["records"]), dtype=np.int32), e["records"])
    return st


def _last(e, st, th):
    return dict(store=st, slot=e["slot"], octave=e["octave"], angle=e["angle"], Tcw_pred=e["Tcw_pred"], th=th)


def _host(capi, e, th):
    return capi.build_frame_queries_host(dict(e, th=th), rs.K, rs.BOUNDS, rs.SCALE, e["records"])


@pytest.mark.parametrize("mode", ["all", "none", "mix"])
@pytest.mark.parametrize("n", COUNTS)
def test_queries_equal_host_bit_for_bit(rig, n, mode):
    capi, trk = rig
    e = rs.entries(n, mode, seed=1000 + 7 * n + len(mode), store_cap=max(n, 1) + 17)
    st = _store(capi, e)
    dev = trk.debug_build_queries([_last(e, st, 15.0)], rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)[0]
    host = _host(capi, e, 15.0)
    rs.assert_queries_equal(dev, host)
    assert dev["nq"] == int((e["fate"] == 0).sum())            # the fates the scene was built with
    if mode == "all":
        assert dev["nq"] == n and np.array_equal(dev["q_entry"], np.arange(n))
    if mode == "none":
        assert dev["nq"] == 0
    if mode == "mix" and n >= 255:
        assert 0 < dev["nq"] < n and all((e["fate"] == f).any() for f in range(6))
        assert (dev["q_claims"] == 0).any() and (dev["q_claims"] == 1).any()
        assert dev["qmin"].min() == -1 or dev["qmax"].max() == rs.NLEVELS       # octave 0 or nlevels - 1 among the kept
    st.close()


def test_batch_of_three_equals_single_calls(rig):
    """Three frames with different n (one of them 0), different stores, poses and th in one launch: frame b equals the single call."""
    capi, trk = rig
    es = [rs.entries(300, "mix", 51), rs.entries(0, "all", 52), rs.entries(77, "all", 53)]
    ths = [15.0, 7.0, 30.0]
    sts = [_store(capi, e) for e in es]
    lasts = [_last(e, st, th) for e, st, th in zip(es, sts, ths)]
    batch = trk.debug_build_queries(lasts, rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)
    for b in range(3):
        single = trk.debug_build_queries([lasts[b]], rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)[0]
        rs.assert_queries_equal(batch[b], single)
        rs.assert_queries_equal(batch[b], _host(capi, es[b], ths[b]))
    assert [b["nq"] for b in batch][1:] == [0, 77] and 0 < batch[0]["nq"] < 300
    for st in sts:
        st.close()


def test_doubled_th_changes_the_radius_only(rig):
    capi, trk = rig
    e = rs.entries(257, "mix", 61)
    st = _store(capi, e)
    a = trk.debug_build_queries([_last(e, st, 15.0)], rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)[0]
    w = trk.debug_build_queries([_last(e, st, 30.0)], rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)[0]
    rs.assert_queries_equal(a, w, skip=("qr",))                # the kept set and every other array unchanged
    host_w = _host(capi, e, 30.0)
    assert w["qr"].tobytes() == host_w["qr"].tobytes()         # exactly the host's doubled-window radius
    assert not np.array_equal(a["qr"], w["qr"])
    st.close()


def test_the_store_is_what_is_read(rig):
    """An update between two calls moves the queries; the slots it does not name keep theirs."""
    capi, trk = rig
    e = rs.entries(200, "all", 71)
    st = _store(capi, e)
    a = trk.debug_build_queries([_last(e, st, 15.0)], rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)[0]
    moved = e["slot"][:30]
    rec = e["records"].copy()
    rec["pos"][moved, 0] += np.float32(0.05)
    rec["n_obs"][moved[:10]] = np.where(rec["n_obs"][moved[:10]] > 0, 0, 2)
    st.update(moved, rec[moved])
    b = trk.debug_build_queries([_last(e, st, 15.0)], rs.K, rs.BOUNDS, rs.SCALE, rs.INV_S2)[0]
    rs.assert_queries_equal(b, _host(capi, dict(e, records=rec), 15.0))
    assert b["nq"] == a["nq"] == 200
    assert np.all(b["qx"][:30] != a["qx"][:30]) and np.array_equal(b["qx"][30:], a["qx"][30:])
    assert np.all(b["q_claims"][:10] != a["q_claims"][:10])
    st.close()
