"""Without a GPU every entry point that needs one returns DVM_ERR_NO_DEVICE (-5) with ONE message, whichever source file it lives in;
a constructor leaves *out null; and an entry point that refuses a bad argument before it looks for a device still does so."""
import ctypes as C

import numpy as np
import pytest

NO_DEVICE, INVALID = -5, -1
MESSAGE = b"no HIP device visible (libdvmslam_hip has no CPU path)"
i32, f32, vp = C.c_int32, C.c_float, C.c_void_p


@pytest.fixture(scope="module")
def L(capi):
    if capi.device_count() > 0:
        pytest.skip("a GPU is visible")
    lib = C.CDLL(capi.LIB_PATH)      # the same library, its functions without capi's argtypes: every argument below is typed at the call
    lib.dvm_last_error.restype = C.c_char_p
    return lib


def _ptr(a):
    return vp(a.ctypes.data)


def _refused(L, rc):
    assert rc == NO_DEVICE
    assert L.dvm_last_error() == MESSAGE


def test_constructors(L, capi):
    z = np.zeros(64, np.float64)     # any non-null array: nothing is read before the device check, or only its zeros
    params = capi.OrbParams(1000, 1.2, 8, 20, 7)
    child_off = np.zeros(2, np.int32)
    creates = [
        ("dvm_orb_create", (C.byref(params), i32(0), i32(1))),                         # orb_pipeline.cpp
        ("dvm_frame_create", (i32(0), i32(1000), i32(1))),                             # capi.cpp
        ("dvm_match_pool_create", (i32(0), i32(4), i32(1000), i32(1000), i32(0))),     # capi.cpp
        ("dvm_bowdb_create", (i32(0),)),                                               # capi.cpp
        ("dvm_vocab_create", (i32(0), i32(1), _ptr(child_off), _ptr(z), _ptr(z), _ptr(z), _ptr(z), i32(0))),   # capi.cpp
        ("dvm_ba_create", (i32(0),)),                                                  # ba_solver.cpp
        ("dvm_pose_pool_create", (i32(0), i32(4), i32(0))),                            # orb_pool.cpp
        ("dvm_tracker_create", (i32(0), i32(1000), i32(1000))),                        # track.cpp
        ("dvm_new_points_create", (i32(0),)),                                          # new_points.cpp
        ("dvm_fuse_targets_create", (i32(0),)),                                        # fuse_targets.cpp
    ]
    for name, args in creates:
        out = vp(0xdead)
        _refused(L, getattr(L, name)(*args, C.byref(out)))
        assert not out.value, name


def test_count_only_entry_points(L):
    z = np.zeros(256, np.float64)
    # dvm_is_in_frustum(frame, P, normal, min_dist, max_dist, n, viewing_cos_limit, out, on_device, stream)
    _refused(L, L.dvm_is_in_frustum(_ptr(z), _ptr(z), _ptr(z), _ptr(z), _ptr(z), i32(1), f32(0.5), _ptr(z), i32(0), vp(0)))
    # dvm_undistort_keypoints(cam, kps_in, kps_out, n, on_device, stream)
    cam = np.array([500, 500, 320, 240, 0.1, 0, 0, 0, 0], np.float32)
    _refused(L, L.dvm_undistort_keypoints(_ptr(cam), _ptr(z), _ptr(z), i32(1), i32(0), vp(0)))
    # dvm_triangulate_matches(pair, kps1, n1, kps2, n2, pairs, n, sigma2_1, sigma2_2, scale_1, scale_2, x3D, status, on_device, stream)
    pair = np.zeros(1, np.dtype([("cos", "f8"), ("K1", "f4", 4), ("K2", "f4", 4), ("T", "f4", 24), ("Ow", "f4", 6), ("rf", "f4"), ("far", "f4"),
                                 ("far_points", "i4"), ("n_levels", "i4")]))
    pair["K1"] = pair["K2"] = (500, 500, 320, 240); pair["n_levels"] = 8
    tri = (_ptr(z), i32(1), _ptr(z), i32(1), _ptr(z), i32(1), _ptr(z), _ptr(z), _ptr(z), _ptr(z), _ptr(z), _ptr(z), i32(0), vp(0))
    _refused(L, L.dvm_triangulate_matches(_ptr(pair), *tri))
    # dvm_pose_graph_optimize(device, S, fixed, n, edges, E, fix_scale, iterations, stats)                        pg_solver.cpp
    _refused(L, L.dvm_pose_graph_optimize(i32(0), _ptr(z), _ptr(z), i32(2), _ptr(z), i32(1), i32(1), i32(1), vp(0)))
    # dvm_pose_graph_debug_trial(device, S, fixed, n, edges, E, fix_scale, lambda, e, J, H, b, x, vidx, stats)      pg_solver.cpp
    _refused(L, L.dvm_pose_graph_debug_trial(i32(0), _ptr(z), _ptr(z), i32(2), _ptr(z), i32(1), i32(1), C.c_double(1.0), _ptr(z), _ptr(z), _ptr(z),
                                             _ptr(z), _ptr(z), _ptr(z), _ptr(z)))
    # dvm_tile_solve_debug(device, n_blocks, dof, per_tile, n_kept, kept_list, n_landmarks, A, b, mask, x_in, form, repeats, A2, b2, x, fail, x2, fail2, info)   tile_debug.cpp
    _refused(L, L.dvm_tile_solve_debug(i32(0), i32(1), i32(6), i32(10), i32(0), vp(0), i32(0), _ptr(z), _ptr(z), vp(0), _ptr(z), i32(0), i32(1), vp(0),
                                       vp(0), _ptr(z), _ptr(z), vp(0), vp(0), _ptr(z)))
    # dvm_wire_gather_keypoints(d_block, first_kf, count, d_kps, kps_stride, d_desc, desc_stride, stream)         wire.cpp
    _refused(L, L.dvm_wire_gather_keypoints(vp(64), i32(0), i32(1), vp(64), C.c_int64(1), vp(64), C.c_int64(32), vp(0)))

    # the argument checks come first: a bad argument is DVM_ERR_INVALID here too, not DVM_ERR_NO_DEVICE
    cam[0] = 0      # zero focal length
    assert L.dvm_undistort_keypoints(_ptr(cam), _ptr(z), _ptr(z), i32(1), i32(0), vp(0)) == INVALID
    assert L.dvm_last_error() == b"dvm_undistort_keypoints: zero focal length"
    pair["n_levels"] = 65
    assert L.dvm_triangulate_matches(_ptr(pair), *tri) == INVALID
    assert L.dvm_last_error() == b"dvm_triangulate_matches: n_levels out of range"
    assert L.dvm_is_in_frustum(_ptr(z), vp(0), _ptr(z), _ptr(z), _ptr(z), i32(1), f32(0.5), _ptr(z), i32(0), vp(0)) == INVALID
    assert L.dvm_tile_solve_debug(i32(0), i32(1), i32(6), i32(9), i32(0), vp(0), i32(0), _ptr(z), _ptr(z), vp(0), _ptr(z), i32(0), i32(1), vp(0), vp(0),
                                  _ptr(z), _ptr(z), vp(0), vp(0), _ptr(z)) == INVALID          # (6, 9) is neither layout
    assert L.dvm_last_error() == b"dvm_tile_solve_debug: bad arguments"
