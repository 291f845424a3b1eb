"""dvm_map_store (capi.MapStore): an agent's map points resident on the device.  Records written through update() come back byte for byte
through read(); a second update changes exactly the slots it names; stores are independent; a slot outside the store, a slot named twice,
a NULL argument and a slot never written are refused on the host with DVM_ERR_INVALID and nothing is written."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 200
INVALID = -1


def _records(capi, n, rng):
    r = np.zeros(n, capi.LOCAL_POINT_DTYPE)
    r.view(np.uint8)[:] = rng.integers(0, 256, n * capi.LOCAL_POINT_DTYPE.itemsize, dtype=np.uint8)   # every byte of the 72 is carried
    return r


def _code(capi, fn):
    with pytest.raises(capi.DvmError) as e:
        fn()
    return e.value.code


def _same(a, b):
    return a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_update_then_read_byte_for_byte(n):
    from dvm_slam_amd import capi
    assert capi.LOCAL_POINT_DTYPE.itemsize == 72
    rng = np.random.default_rng(100 + n)
    st = capi.MapStore(CAP)
    assert st.capacity == CAP
    slots = rng.permutation(CAP)[:n].astype(np.int32)          # shuffled order
    rec = _records(capi, n, rng)
    st.update(slots, rec)
    assert _same(st.read(slots), rec)
    order = rng.permutation(n)
    assert _same(st.read(slots[order]), rec[order])            # any order, and a slot may repeat in a read
    assert _same(st.read(np.concatenate([slots, slots])), np.concatenate([rec, rec]))
    st.close()


def test_second_update_changes_exactly_its_slots_and_stores_are_independent():
    from dvm_slam_amd import capi
    rng = np.random.default_rng(7)
    a, b = capi.MapStore(CAP), capi.MapStore(CAP)
    all_slots = np.arange(CAP, dtype=np.int32)
    ra, rb = _records(capi, CAP, rng), _records(capi, CAP, rng)
    a.update(all_slots, ra)
    b.update(all_slots[::-1].copy(), rb[::-1].copy())
    sub = rng.permutation(CAP)[:37].astype(np.int32)
    new = _records(capi, len(sub), rng)
    a.update(sub, new)                                         # two updates back to back: the second waits for the staging block
    a.update(sub[:5], new[:5])
    want = ra.copy(); want[sub] = new
    assert _same(a.read(all_slots), want)
    assert _same(b.read(all_slots), rb)                        # the other store saw nothing
    a.close()
    assert _same(b.read(all_slots), rb)
    b.close()


def test_error_paths_write_nothing():
    from dvm_slam_amd import capi
    rng = np.random.default_rng(9)
    st = capi.MapStore(CAP)
    written = np.arange(0, 100, dtype=np.int32)
    rec = _records(capi, 100, rng)
    st.update(written, rec)
    other = _records(capi, 3, rng)
    assert _code(capi, lambda: st.update(np.array([5, -1, 6], np.int32), other)) == INVALID           # slot -1
    assert _code(capi, lambda: st.update(np.array([5, CAP, 6], np.int32), other)) == INVALID          # slot = capacity
    assert _code(capi, lambda: st.update(np.array([5, 150, 5], np.int32), other)) == INVALID          # a slot named twice
    assert _same(st.read(written), rec)                                                              # nothing was written ...
    assert _code(capi, lambda: st.read(np.array([150], np.int32))) == INVALID                         # ... not even the valid slot of a refused call
    assert _code(capi, lambda: st.read(np.array([3, 100], np.int32))) == INVALID                      # read naming an unwritten slot
    assert _code(capi, lambda: st.read(np.array([CAP], np.int32))) == INVALID
    # NULL arguments, through the C ABI
    L = capi.lib()
    L.dvm_map_store_update.restype = C.c_int32; L.dvm_map_store_update.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.dvm_map_store_read.restype = C.c_int32; L.dvm_map_store_read.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.dvm_map_store_create.restype = C.c_int32; L.dvm_map_store_create.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
    s3 = np.array([1, 2, 3], np.int32)
    assert L.dvm_map_store_update(None, 3, s3.ctypes.data, other.ctypes.data) == INVALID
    assert L.dvm_map_store_update(st.h, 3, None, other.ctypes.data) == INVALID
    assert L.dvm_map_store_update(st.h, 3, s3.ctypes.data, None) == INVALID
    assert L.dvm_map_store_read(st.h, 3, None, other.ctypes.data) == INVALID
    assert L.dvm_map_store_read(st.h, 3, s3.ctypes.data, None) == INVALID
    assert L.dvm_map_store_create(0, CAP, None) == INVALID
    h = C.c_void_p()
    assert L.dvm_map_store_create(0, 0, C.byref(h)) == INVALID and not h.value
    assert _same(st.read(written), rec)
    st.close()


def test_chain_calls_refuse_unwritten_slots():
    """The builder of the resident first half names a slot never written (and one outside the store): DVM_ERR_INVALID before anything runs."""
    from dvm_slam_amd import capi
    rng = np.random.default_rng(11)
    ext = capi.OrbExtractor(max_batch=1)
    tab = ext.tables()
    trk = capi.Tracker(ext)
    st = capi.MapStore(CAP)
    st.update(np.arange(50, dtype=np.int32), _records(capi, 50, rng))
    K = np.array([500.0, 510.0, 320.0, 240.0], np.float32)
    B4 = np.array([0, 640, 0, 480], np.float32)

    def last(slots):
        n = len(slots)
        return dict(store=st, slot=np.asarray(slots, np.int32), octave=np.zeros(n, np.uint8), angle=np.zeros(n, np.float32),
                    Tcw_pred=np.array([0, 0, 0, 1, 0, 0, 0], np.float32), th=15.0)
    trk.debug_build_queries([last([0, 49])], K, B4, tab["scale"], tab["inv_sigma2"])                 # written slots pass
    assert _code(capi, lambda: trk.debug_build_queries([last([0, 50])], K, B4, tab["scale"], tab["inv_sigma2"])) == INVALID
    assert _code(capi, lambda: trk.debug_build_queries([last([0, CAP])], K, B4, tab["scale"], tab["inv_sigma2"])) == INVALID
    assert _code(capi, lambda: trk.debug_build_queries([last([-1])], K, B4, tab["scale"], tab["inv_sigma2"])) == INVALID
    st.close(); trk.close(); ext.close()
