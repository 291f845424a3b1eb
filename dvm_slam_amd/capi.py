"""ctypes binding of libdvmslam_hip.so (include/dvmslam_hip.h).

This is the only way Python (tests, bench.py, smoke) reaches the product: through the C ABI a
reference maintainer would bind.  There is NO CPU fallback: if the shared library is missing the
import raises, and on a box without a gfx950 device every compute entry point returns
DVM_ERR_NO_DEVICE (raised here as DvmError).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DVM_HIP_LIB") or os.path.join(_HERE, "lib", "libdvmslam_hip.so")   # (DVM_HIP_LIB: a measurement build, tools/build_flow_stamps.sh)

DVM_OK = 0
ERRORS = {-1: "DVM_ERR_INVALID", -2: "DVM_ERR_EMPTY", -3: "DVM_ERR_CAPACITY", -4: "DVM_ERR_HIP",
          -5: "DVM_ERR_NO_DEVICE", -6: "DVM_ERR_STATE"}

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
MATCH_DTYPE = np.dtype([("best_idx", "<i4"), ("best_dist", "<i4"), ("second_dist", "<i4"),
                        ("best_level", "<i2"), ("second_level", "<i2")])


class DvmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


BA_EDGE_DTYPE = np.dtype([("pose", "<i4"), ("point", "<i4"), ("u", "<f8"), ("v", "<f8"), ("inv_sigma2", "<f8")])


class BaCamera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("huber_delta", C.c_double)]


class BaStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("total_trials", C.c_int32), ("stop_reason", C.c_int32), ("kernel_us", C.c_int32),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double),
                ("trials_per_iter", C.c_int32 * 64), ("chi2_per_iter", C.c_double * 64),
                ("lambda_per_iter", C.c_double * 64), ("ms_structure", C.c_double), ("ms_optimize", C.c_double),
                ("spec_trials", C.c_int32), ("spec_kept", C.c_int32)]


class FrustumFrame(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float), ("bf", C.c_float), ("log_scale_factor", C.c_float), ("n_levels", C.c_int32)]


class CameraModel(C.Structure):   # == dvm_camera_model
    """A camera model of the reference's GeometricCamera: model 0 pinhole, 1 KannalaBrandt8; p = fx, fy, cx, cy, k1, k2, k3, k4."""
    _fields_ = [("model", C.c_int32), ("p", C.c_float * 8)]
    PINHOLE, KANNALA_BRANDT8 = 0, 1

    @classmethod
    def make(cls, model, params):
        v = [float(x) for x in params] + [0.0] * (8 - len(params))
        return cls(int(model), (C.c_float * 8)(*v))

    @classmethod
    def pinhole(cls, fx, fy, cx, cy):
        return cls.make(cls.PINHOLE, [fx, fy, cx, cy])

    @classmethod
    def robomaster(cls):
        """The real robot's camera (Camera.type: "KannalaBrandt8"): calibrated at 1920 x 1080 and used at 960 x 540, so fx, fy, cx, cy are
        the calibration's times 0.5, as the reference's Settings scale them for the resized image."""
        return cls.make(cls.KANNALA_BRANDT8, [0.5 * 495.1139105110322, 0.5 * 494.58353174914896, 0.5 * 960.3182783342162, 0.5 * 555.0427286112108,
                                              -0.027058405982580736, 0.025005319766890292, -0.02255121102967952, 0.006475379139360301])

    @classmethod
    def tum(cls):
        """The 512 x 512 fisheye camera of the TUM-VI sequences (Camera.type: "KannalaBrandt8")."""
        return cls.make(cls.KANNALA_BRANDT8, [190.978477, 190.973307, 254.931706, 256.897442, 0.003482389402, 0.000715034845, -0.002053236141, 0.000202936736])

    @property
    def params(self):
        return np.array(list(self.p), np.float32)

    def project(self, Xc):
        """Pixels of camera-frame points [n, 3] in float64 (for building scenes; the device code is csrc/camera_model.h)."""
        p = self.params.astype(np.float64); X = np.asarray(Xc, np.float64).reshape(-1, 3)
        if self.model == self.PINHOLE:
            return np.stack([p[0] * X[:, 0] / X[:, 2] + p[2], p[1] * X[:, 1] / X[:, 2] + p[3]], axis=1)
        rho = np.hypot(X[:, 0], X[:, 1]); th = np.arctan2(rho, X[:, 2])
        r = th * (1 + th ** 2 * (p[4] + th ** 2 * (p[5] + th ** 2 * (p[6] + th ** 2 * p[7]))))
        with np.errstate(invalid="ignore", divide="ignore"):
            c, s = np.where(rho > 0, X[:, 0] / rho, 1.0), np.where(rho > 0, X[:, 1] / rho, 0.0)
        return np.stack([p[0] * r * c + p[2], p[1] * r * s + p[3]], axis=1)


class TriPair(C.Structure):   # == dvm_tri_pair
    _fields_ = [("cos_parallax_max", C.c_double), ("K1", C.c_float * 4), ("K2", C.c_float * 4), ("T1w", C.c_float * 12), ("T2w", C.c_float * 12),
                ("Ow1", C.c_float * 3), ("Ow2", C.c_float * 3), ("ratio_factor", C.c_float), ("th_far", C.c_float), ("far_points", C.c_int32),
                ("n_levels", C.c_int32)]


TRACK_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("depth", "<f4"), ("view_cos", "<f4"),
                        ("level", "<i4"), ("in_view", "<i4")])

_LIB = None


def lib():
    """Loads the HIP library; raises if it has not been built (no silent fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); dvm_slam_amd has no CPU implementation")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same soname as
    # /opt/rocm's).  Whichever is loaded first serves both; loading torch AFTER us would pull a second
    # runtime in and neither would see the GPU.  So when torch is importable, import it first.
    if os.environ.get("DVM_NO_TORCH_PRELOAD", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    L.dvm_last_error.restype = C.c_char_p
    L.dvm_version.restype = C.c_char_p
    L.dvm_device_count.restype = i32
    L.dvm_orb_create.argtypes = [C.POINTER(OrbParams), i32, i32, C.POINTER(vp)]
    L.dvm_orb_destroy.argtypes = [vp]
    L.dvm_orb_destroy.restype = None
    L.dvm_orb_tables.argtypes = [vp] * 6
    L.dvm_orb_extract.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp]
    L.dvm_orb_extract_batch_device.argtypes = [vp, vp, i32, i32, i32, i32, i64, i32, i32]
    L.dvm_orb_extract_batch_host.argtypes = [vp, vp, i32, i32, i32, i32, i64, i32, i32]
    L.dvm_orb_sync.argtypes = [vp]
    L.dvm_orb_result_device.argtypes = [vp, i32, vp, vp, vp, vp]
    L.dvm_orb_copy_result.argtypes = [vp, i32, vp, vp, vp]
    L.dvm_orb_scale_factors_device.argtypes = [vp]
    L.dvm_orb_scale_factors_device.restype = vp
    L.dvm_orb_download.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    L.dvm_orb_pyramid.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.dvm_orb_debug_level.argtypes = [vp, i32, i32, i32, vp]
    L.dvm_orb_debug_blurred.argtypes = [vp, i32, i32, vp]
    L.dvm_orb_debug_candidates.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp]
    L.dvm_orb_debug_level_keypoints.argtypes = [vp, i32, i32, vp, i32, vp]
    L.dvm_orb_profiling.argtypes = [vp, i32]
    L.dvm_orb_profile_get.argtypes = [vp, C.c_char_p, vp, vp]
    L.dvm_orb_profile_reset.argtypes = [vp]
    L.dvm_orb_stream.argtypes = [vp]
    L.dvm_orb_stream.restype = vp
    L.dvm_hamming_matrix.argtypes = [vp, i32, vp, i32, vp, i32, vp]
    L.dvm_frame_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.dvm_frame_destroy.argtypes = [vp]
    L.dvm_frame_destroy.restype = None
    L.dvm_frame_build.argtypes = [vp, i32, vp, vp, i32, vp, f32, f32, f32, f32, i32, vp]
    L.dvm_frame_build_batch.argtypes = [vp, i32, i32, vp, i64, vp, i64, vp, f32, f32, f32, f32, vp]
    L.dvm_match_window.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, vp]
    L.dvm_is_in_frustum.argtypes = [C.POINTER(FrustumFrame), vp, vp, vp, vp, i32, f32, vp, i32, vp]
    L.dvm_undistort_keypoints.argtypes = [vp, vp, vp, i32, i32, vp]
    L.dvm_image_bounds.argtypes = [vp, i32, i32, vp]
    L.dvm_match_lists.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, vp]
    L.dvm_match_frames_batch.argtypes = [vp, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, i32, f32, vp, i32, vp, i64,
                                         vp, vp]
    L.dvm_ba_create.argtypes = [i32, C.POINTER(vp)]
    L.dvm_ba_destroy.argtypes = [vp]
    L.dvm_ba_destroy.restype = None
    L.dvm_ba_set_problem.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, C.POINTER(BaCamera)]
    L.dvm_ba_optimize.argtypes = [vp, i32, vp, C.POINTER(BaStats)]
    L.dvm_ba_get_result.argtypes = [vp, vp, vp]
    L.dvm_ba_edge_chi2.argtypes = [vp, vp, vp]
    L.dvm_ba_stream.argtypes = [vp]
    L.dvm_ba_stream.restype = vp
    L.dvm_optimize_sim3.argtypes = [i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, C.c_double, vp, vp]
    L.dvm_pose_optimize.argtypes = [i32, vp, vp, vp, vp, vp, i32, i32, C.POINTER(BaCamera), vp, vp, vp]
    _declare(L, _TRACK_API)
    _LIB = L
    return L


def check(rc):
    if rc != DVM_OK:
        raise DvmError(rc, lib().dvm_last_error().decode(errors="replace"))


def device_count() -> int:
    return int(lib().dvm_device_count())


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a))


class OrbExtractor:
    """Mirror of ORB_SLAM3::ORBextractor (reference include/ORBextractor.h:47-91) over the C ABI."""

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, device=0, max_batch=1):
        self.L = lib()
        self.h = C.c_void_p()
        self.params = OrbParams(nfeatures, scale_factor, nlevels, ini_th, min_th)
        self.nlevels, self.nfeatures, self.max_batch = nlevels, nfeatures, max_batch
        check(self.L.dvm_orb_create(C.byref(self.params), device, max_batch, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.dvm_orb_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def tables(self):
        n = self.nlevels
        sc, isc, s2, is2 = (np.zeros(n, np.float32) for _ in range(4))
        nf = np.zeros(n, np.int32)
        check(self.L.dvm_orb_tables(self.h, _p(sc), _p(isc), _p(s2), _p(is2), _p(nf)))
        return dict(scale=sc, inv_scale=isc, sigma2=s2, inv_sigma2=is2, nfeat=nf)

    @property
    def cap(self):
        return self.nfeatures + 5 * self.nlevels + 8

    def last_result(self):
        """dvm_orb_last_result: a DeviceFrame naming the keypoints + descriptors of the last extract(), still in HBM."""
        r = DeviceFrame()
        f = self.L.dvm_orb_last_result
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.h, C.byref(r)))
        return r

    def extract(self, img: np.ndarray, lap=(0, 1000)):
        """operator(): returns (n, keypoints, descriptors, monoIndex); n == -1 for an empty image."""
        if img is None or img.size == 0:
            rc = self.L.dvm_orb_extract(self.h, None, 0, 0, 0, lap[0], lap[1], None, None, 0, None, None)
            assert rc == -2, rc
            return -1, None, None, -1
        if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1:
            img = np.ascontiguousarray(img, np.uint8)  # row-strided views (stride > cols) pass through as they are
        kps = np.empty(self.cap, KP_DTYPE)          # (the call fills [0, n); the rest is never looked at)
        desc = np.empty((self.cap, 32), np.uint8)
        n, mono = C.c_int(0), C.c_int(0)
        rc = self.L.dvm_orb_extract(self.h, _p(img), img.shape[0], img.shape[1], img.strides[0], lap[0], lap[1],
                                    _p(kps), _p(desc), self.cap, C.byref(n), C.byref(mono))
        if rc == -3 and n.value > self.cap:   # DVM_ERR_CAPACITY: *n holds the size needed (small quotas on wide images)
            return self.download(0, cap=n.value)
        check(rc)
        return n.value, kps[:n.value], desc[:n.value], mono.value

    def extract_batch_host(self, imgs: np.ndarray, lap=(0, 1000)):
        imgs = np.ascontiguousarray(imgs, np.uint8)
        b, r, c = imgs.shape
        check(self.L.dvm_orb_extract_batch_host(self.h, _p(imgs), b, r, c, imgs.strides[1], imgs.strides[0], lap[0], lap[1]))

    def extract_batch_device(self, d_ptr: int, batch, rows, cols, stride=None, frame_stride=None, lap=(0, 1000)):
        stride = stride or cols
        frame_stride = frame_stride or rows * stride
        check(self.L.dvm_orb_extract_batch_device(self.h, C.c_void_p(d_ptr), batch, rows, cols, stride, frame_stride,
                                                  lap[0], lap[1]))

    def staging(self, batch, rows, cols) -> np.ndarray:
        """The handle's pinned input buffer as a (batch, rows, cols) uint8 array (dvm_orb_staging); waits for the previous copy."""
        p = C.c_void_p()
        f = self.L.dvm_orb_staging
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.h, C.c_int32(batch), C.c_int32(rows), C.c_int32(cols), C.byref(p)))
        buf = (C.c_uint8 * (batch * rows * cols)).from_address(p.value)
        return np.frombuffer(buf, np.uint8).reshape(batch, rows, cols)

    def extract_staged(self, batch, rows, cols, lap=(0, 1000)):
        f = self.L.dvm_orb_extract_staged
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.h, C.c_int32(batch), C.c_int32(rows), C.c_int32(cols), C.c_int32(lap[0]), C.c_int32(lap[1])))

    def sync(self):
        check(self.L.dvm_orb_sync(self.h))

    def download(self, frame=0, cap=None):
        cap = cap or self.cap
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n, mono = C.c_int(0), C.c_int(0)
        rc = self.L.dvm_orb_download(self.h, frame, _p(kps), _p(desc), cap, C.byref(n), C.byref(mono))
        if rc == -3 and n.value > cap:
            return self.download(frame, cap=n.value)
        check(rc)
        return n.value, kps[:n.value].copy(), desc[:n.value].copy(), mono.value

    def result_device(self, frame=0):
        k, d, n = C.c_void_p(), C.c_void_p(), C.c_void_p()
        cap = C.c_int(0)
        check(self.L.dvm_orb_result_device(self.h, frame, C.byref(k), C.byref(d), C.byref(n), C.byref(cap)))
        return k.value, d.value, n.value, cap.value

    def copy_result(self, frame, d_kps, d_desc, d_n):
        check(self.L.dvm_orb_copy_result(self.h, frame, C.c_void_p(d_kps), C.c_void_p(d_desc), C.c_void_p(d_n)))

    def scale_factors_device(self):
        return self.L.dvm_orb_scale_factors_device(self.h)

    def pyramid(self, frame, level):
        ptr = C.c_void_p()
        r, c, s = C.c_int(0), C.c_int(0), C.c_int(0)
        check(self.L.dvm_orb_pyramid(self.h, frame, level, C.byref(ptr), C.byref(r), C.byref(c), C.byref(s)))
        return ptr.value, r.value, c.value, s.value

    def debug_level(self, frame, level, bordered=False):
        _, r, c, _ = self.pyramid(frame, level)
        out = np.zeros((r + 38, c + 38) if bordered else (r, c), np.uint8)
        check(self.L.dvm_orb_debug_level(self.h, frame, level, int(bordered), _p(out)))
        return out

    def debug_pyr_path(self, level) -> int:
        """1 if the last batch built this level with k_pyr_resize_direct, 0 for k_pyr_resize (dvm_orb_debug_pyr_path)."""
        out = C.c_int(0)
        f = self.L.dvm_orb_debug_pyr_path
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.h, C.c_int32(level), C.byref(out)))
        return out.value

    def debug_blurred(self, frame, level):
        _, r, c, _ = self.pyramid(frame, level)
        out = np.zeros((r, c), np.uint8)
        check(self.L.dvm_orb_debug_blurred(self.h, frame, level, _p(out)))
        return out

    def debug_candidates(self, frame, level, cap=300000):
        xs, ys, sc = (np.zeros(cap, np.int32) for _ in range(3))
        n = C.c_int(0)
        check(self.L.dvm_orb_debug_candidates(self.h, frame, level, _p(xs), _p(ys), _p(sc), cap, C.byref(n)))
        return xs[:n.value].copy(), ys[:n.value].copy(), sc[:n.value].copy()

    def debug_level_keypoints(self, frame, level, cap=20000):
        k = np.zeros(cap, KP_DTYPE)
        n = C.c_int(0)
        check(self.L.dvm_orb_debug_level_keypoints(self.h, frame, level, _p(k), cap, C.byref(n)))
        return k[:n.value].copy()

    def profiling(self, on=True):
        """True / 1: HIP events around every stage; 2: around the dominant kernel (k_fast_cells) only -- an event record is a marker
        packet between two kernels of the batch, a few microseconds of idle device each; False / 0: none."""
        check(self.L.dvm_orb_profiling(self.h, int(on)))

    def profile_reset(self):
        check(self.L.dvm_orb_profile_reset(self.h))

    def profile_get(self, name):
        ms, cnt = C.c_double(0), C.c_int64(0)
        rc = self.L.dvm_orb_profile_get(self.h, name.encode(), C.byref(ms), C.byref(cnt))
        return (ms.value, cnt.value) if rc == 0 else (0.0, 0)

    def stream(self):
        return self.L.dvm_orb_stream(self.h)


def hamming_matrix(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """All-pairs ORBmatcher::DescriptorDistance (host arrays in, host matrix out)."""
    A = np.ascontiguousarray(A, np.uint8).reshape(-1, 32)
    B = np.ascontiguousarray(B, np.uint8).reshape(-1, 32)
    D = np.zeros((len(A), len(B)), np.uint16)
    check(lib().dvm_hamming_matrix(_p(A), len(A), _p(B), len(B), _p(D), 0, None))
    return D


def match_lists(tdesc: np.ndarray, qdesc: np.ndarray, offsets: np.ndarray, cand: np.ndarray) -> np.ndarray:
    """Best / second best of query q over train indices cand[offsets[q]:offsets[q+1]] (list order = tie order)."""
    tdesc = np.ascontiguousarray(tdesc, np.uint8).reshape(-1, 32)
    qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    offsets = np.ascontiguousarray(offsets, np.int32)
    cand = np.ascontiguousarray(cand, np.int32)
    out = np.zeros(len(qdesc), MATCH_DTYPE)
    check(lib().dvm_match_lists(_p(tdesc), len(tdesc), _p(qdesc), len(qdesc), _p(offsets), _p(cand), _p(out), 0, None))
    return out


class OrbPool:
    """dvm_orb_pool_*: one extractor shared by several agents' threads; frames arriving together are extracted as one batch."""

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, max_batch=32, window_us=-1, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        p = OrbParams(nfeatures, scale_factor, nlevels, ini_th, min_th)
        f = self.L.dvm_orb_pool_create
        f.restype = C.c_int32; f.argtypes = None
        check(f(C.byref(p), C.c_int32(device), C.c_int32(max_batch), C.c_int32(window_us), C.byref(self.h)))
        self.cap = 4 * max(nfeatures, 1) + 256   # (small quotas on wide images keep up to 4 * nIni keypoints per level)
        self._x = self.L.dvm_orb_pool_extract
        self._x.restype = C.c_int32; self._x.argtypes = None

    def extract(self, img, lap=(0, 1000)):
        """One frame (blocking, from any thread): (n, keypoints, descriptors, monoIndex, frames in the batch this call ran in)."""
        if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1:
            img = np.ascontiguousarray(img, np.uint8)
        kps = np.empty(self.cap, KP_DTYPE)
        desc = np.empty((self.cap, 32), np.uint8)
        n, mono, bs = C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._x(self.h, _p(img), C.c_int32(img.shape[0]), C.c_int32(img.shape[1]), C.c_int32(img.strides[0]), C.c_int32(lap[0]), C.c_int32(lap[1]),
                      _p(kps), _p(desc), C.c_int32(self.cap), C.byref(n), C.byref(mono), C.byref(bs)))
        return n.value, kps[:n.value], desc[:n.value], mono.value, bs.value

    def close(self):
        if self.h:
            f = self.L.dvm_orb_pool_destroy
            f.restype = None; f.argtypes = None
            f(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PosePool:
    """dvm_pose_pool_*: PoseOptimization of one frame per call, from any thread; calls arriving together run as one launch."""

    def __init__(self, max_batch=32, window_us=-1, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        f = self.L.dvm_pose_pool_create
        f.restype = C.c_int32; f.argtypes = None
        check(f(C.c_int32(device), C.c_int32(max_batch), C.c_int32(window_us), C.byref(self.h)))
        self._x = self.L.dvm_pose_pool_optimize
        self._x.restype = C.c_int32; self._x.argtypes = None

    def optimize(self, pose, Xw, obs, inv_sigma2, intrinsics):
        """One frame: pose [7], Xw [n,3], obs [n,2], inv_sigma2 [n].  Returns (pose [7], outlier [n] uint8, n_inliers, frames in the launch)."""
        pose = np.ascontiguousarray(pose, np.float64).reshape(7)
        Xw = np.ascontiguousarray(Xw, np.float64).reshape(-1, 3)
        n = len(Xw)
        obs = np.ascontiguousarray(obs, np.float64).reshape(n, 2)
        w = np.ascontiguousarray(inv_sigma2, np.float64).reshape(n)
        cam = BaCamera(*[float(v) for v in intrinsics], 0.0)
        out = np.zeros(7, np.float64); outl = np.zeros(max(n, 1), np.uint8)
        ninl, bs = C.c_int32(0), C.c_int(0)
        check(self._x(self.h, _p(pose), _p(Xw), _p(obs), _p(w), C.c_int32(n), C.byref(cam), _p(out), _p(outl), C.byref(ninl), C.byref(bs)))
        return out, outl[:n], ninl.value, bs.value

    def close(self):
        if self.h:
            f = self.L.dvm_pose_pool_destroy
            f.restype = None; f.argtypes = None
            f(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MatchPool:
    """dvm_match_pool_*: the grid build + ranked window search of SearchByProjection(Cur, Last) for several threads at once.
    use(): route this process's search_by_projection_frames calls through it (dvmh_set_match_pool); release() / close() undo that."""

    def __init__(self, max_batch=32, kp_cap=2048, q_cap=2048, window_us=-1, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        f = self.L.dvm_match_pool_create
        f.restype = C.c_int32; f.argtypes = None
        check(f(C.c_int32(device), C.c_int32(max_batch), C.c_int32(kp_cap), C.c_int32(q_cap), C.c_int32(window_us), C.byref(self.h)))

    def use(self):
        f = host_lib().dvmh_set_match_pool
        f.restype = None; f.argtypes = [C.c_void_p]
        f(self.h)

    def release(self):
        f = host_lib().dvmh_set_match_pool
        f.restype = None; f.argtypes = [C.c_void_p]
        f(None)

    def close(self):
        if self.h:
            self.release()
            f = self.L.dvm_match_pool_destroy
            f.restype = None; f.argtypes = None
            f(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrameGrid:
    """Frame's feature grid + windowed search (reference Frame.cc:443-506,712-782; ORBmatcher.cc:70-115)."""

    def __init__(self, capacity=2048, slots=1, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.capacity, self.slots = capacity, slots
        check(self.L.dvm_frame_create(device, capacity, slots, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.dvm_frame_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def build(self, kps: np.ndarray, desc: np.ndarray, bounds=(0.0, 640.0, 0.0, 480.0), slot=0):
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        check(self.L.dvm_frame_build(self.h, slot, _p(kps), _p(desc), len(kps), None, *bounds, 0, None))

    def overflows(self):
        """Sticky count of device-side keypoint counts that exceeded the capacity (raises DvmError if non-zero)."""
        n = C.c_int32(0)
        self.L.dvm_frame_overflows.restype = C.c_int32; self.L.dvm_frame_overflows.argtypes = [C.c_void_p, C.c_void_p]
        check(self.L.dvm_frame_overflows(self.h, C.byref(n)))
        return n.value

    def build_batch_device(self, first_slot, count, d_kps, kps_stride, d_desc, desc_stride, d_n, bounds, stream=None):
        check(self.L.dvm_frame_build_batch(self.h, first_slot, count, C.c_void_p(d_kps), kps_stride, C.c_void_p(d_desc),
                                           desc_stride, C.c_void_p(d_n), *bounds, C.c_void_p(stream or 0)))

    def match_window(self, qdesc, qx, qy, qr, qmin, qmax, skip=None, slot=0, top2=False):
        qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        nq = len(qdesc)
        qx, qy, qr = (np.ascontiguousarray(a, np.float32) for a in (qx, qy, qr))
        qmin, qmax = (np.ascontiguousarray(a, np.int32) for a in (qmin, qmax))
        out = np.zeros(nq, MATCH_DTYPE)
        sk = None
        if skip is not None:
            sk = np.zeros(self.capacity, np.uint8)
            sk[:len(skip)] = skip
        if not top2:
            check(self.L.dvm_match_window(self.h, slot, _p(sk), _p(qdesc), _p(qx), _p(qy), _p(qr), _p(qmin), _p(qmax), nq,
                                          None, _p(out), 0, None))
            return out
        second = np.full(nq, -7, np.int32)
        self.L.dvm_match_window_top2.restype = C.c_int
        self.L.dvm_match_window_top2.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_void_p]
        check(self.L.dvm_match_window_top2(self.h, slot, _p(sk), _p(qdesc), _p(qx), _p(qy), _p(qr), _p(qmin), _p(qmax), nq,
                                           None, _p(out), _p(second), 0, None))
        return out, second

    def match_window_ranked(self, qdesc, qx, qy, qr, qmin, qmax, skip=None, slot=0):
        """dvm_match_window_ranked: the four best candidates per query, best first.  Returns (idx [nq,4] int32, -1 past the end; dist [nq,4])."""
        qdesc = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        nq = len(qdesc)
        qx, qy, qr = (np.ascontiguousarray(a, np.float32) for a in (qx, qy, qr))
        qmin, qmax = (np.ascontiguousarray(a, np.int32) for a in (qmin, qmax))
        ranked = np.zeros((nq, 4), np.uint32)
        sk = None
        if skip is not None:
            sk = np.zeros(self.capacity, np.uint8)
            sk[:len(skip)] = skip
        f = self.L.dvm_match_window_ranked
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        check(f(self.h, slot, _p(sk), _p(qdesc), _p(qx), _p(qy), _p(qr), _p(qmin), _p(qmax), nq, _p(ranked), 0, None))
        dist = (ranked >> 16).astype(np.int32)
        idx = np.where(dist < 256, (ranked & 0xFFFF).astype(np.int32), -1)
        return idx, dist

    def match_frames_batch(self, first_slot, count, d_kps, kps_stride, d_desc, desc_stride, d_n, carry, cap, th,
                           d_scale, nlevels, d_out, out_stride, d_nq_out=None, stream=None):
        ck, cd, cn = carry if carry else (0, 0, 0)
        check(self.L.dvm_match_frames_batch(self.h, first_slot, count, C.c_void_p(d_kps), kps_stride, C.c_void_p(d_desc),
                                            desc_stride, C.c_void_p(d_n), C.c_void_p(ck), C.c_void_p(cd), C.c_void_p(cn),
                                            cap, th, C.c_void_p(d_scale), nlevels, C.c_void_p(d_out), out_stride,
                                            C.c_void_p(d_nq_out or 0), C.c_void_p(stream or 0)))


def make_edges(edge_pose, edge_point, obs, inv_sigma2) -> np.ndarray:
    e = np.zeros(len(edge_pose), BA_EDGE_DTYPE)
    e["pose"], e["point"] = edge_pose, edge_point
    e["u"], e["v"] = obs[:, 0], obs[:, 1]
    e["inv_sigma2"] = inv_sigma2
    return e


BA_EDGE_ACTIVE, BA_EDGE_ROBUST = 1, 2     # DVM_BA_EDGE_ACTIVE / DVM_BA_EDGE_ROBUST


class BundleAdjuster:
    """Optimizer::BundleAdjustment / LocalBundleAdjustment numerics (reference Optimizer.cc:55-356,1030-1387)."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        check(self.L.dvm_ba_create(device, C.byref(self.h)))
        self.P = self.Lm = self.E = 0

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.dvm_ba_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def set_problem(self, poses, fixed, points, edges, intrinsics, huber_delta):
        poses = np.ascontiguousarray(poses, np.float64)
        points = np.ascontiguousarray(points, np.float64)
        fixed = np.ascontiguousarray(fixed, np.uint8)
        edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
        cam = BaCamera(*[float(v) for v in intrinsics], float(huber_delta))
        self.P, self.Lm, self.E = len(poses), len(points), len(edges)
        check(self.L.dvm_ba_set_problem(self.h, _p(poses), _p(fixed), self.P, _p(points), self.Lm, _p(edges), self.E,
                                        C.byref(cam)))

    def set_problem_cam(self, poses, fixed, points, edges, model, huber_delta):
        """dvm_ba_set_problem_cam: the problem on a CameraModel.  KannalaBrandt8 runs the tile solver at every size; the pinhole model is
        set_problem with (double)p[0..3]."""
        poses = np.ascontiguousarray(poses, np.float64)
        points = np.ascontiguousarray(points, np.float64)
        fixed = np.ascontiguousarray(fixed, np.uint8)
        edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
        assert isinstance(model, CameraModel)
        f = self.L.dvm_ba_set_problem_cam
        f.restype = C.c_int32; f.argtypes = None
        rc = f(self.h, _p(poses), _p(fixed), C.c_int32(len(poses)), _p(points), C.c_int32(len(points)), _p(edges), C.c_int32(len(edges)),
               C.byref(model), C.c_double(float(huber_delta)))
        if rc == 0:
            self.P, self.Lm, self.E = len(poses), len(points), len(edges)
        check(rc)

    def set_problem_sharded(self, poses, fixed, points, edges, intrinsics, huber_delta, rank, world):
        """BASELINE config 5: the whole problem on every rank, the observations of the landmarks `point % world == rank`
        evaluated here (dvm_ba_set_problem_sharded).  Needs set_allreduce() before optimize()."""
        poses = np.ascontiguousarray(poses, np.float64)
        points = np.ascontiguousarray(points, np.float64)
        fixed = np.ascontiguousarray(fixed, np.uint8)
        edges = np.ascontiguousarray(edges, BA_EDGE_DTYPE)
        cam = BaCamera(*[float(v) for v in intrinsics], float(huber_delta))
        self.P, self.Lm = len(poses), len(points)
        self.E = int((edges["point"] % world == rank).sum())
        f = self.L.dvm_ba_set_problem_sharded
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.h, _p(poses), _p(fixed), C.c_int32(self.P), _p(points), C.c_int32(self.Lm), _p(edges), C.c_int32(len(edges)),
                C.byref(cam), C.c_int32(rank), C.c_int32(world)))

    def schedule_info(self):
        out = (C.c_int64 * 12)()
        f = self.L.dvm_ba_schedule_info
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.h, out))
        keys = ("levels", "columns", "strips", "targets", "products", "products_on_diagonal_targets", "nz_tiles", "ldS", "free_cameras",
                "nz_blocks", "edges", "tiles_per_side")
        return dict(zip(keys, [int(v) for v in out]))

    def solve_info(self):
        out = (C.c_int64 * 6)()
        f = self.L.dvm_ba_solve_info
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.h, out))
        return dict(form="flow" if out[0] else "levels", flow_tasks=int(out[1]), chains=int(out[2]), workgroups=int(out[3]), kept_landmarks=int(out[4]),
                    camera_tiles=int(out[5]))

    def profile(self, enable=-1):
        ms = (C.c_double * 4)(); tr = C.c_int32(0); it = C.c_int32(0)
        f = self.L.dvm_ba_profile
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.h, C.c_int32(enable), ms, C.byref(tr), C.byref(it)))
        return dict(ms_linearise=ms[0], ms_schur=ms[1], ms_cholesky_solve=ms[2], ms_update_chi2=ms[3], trials=tr.value, iterations=it.value)

    def allreduce_doubles(self):
        f = self.L.dvm_ba_allreduce_doubles
        f.restype = C.c_int64; f.argtypes = [C.c_void_p]
        return int(f(self.h))

    ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p)

    def set_allreduce(self, fn, d_buf, cap_doubles):
        """fn(buf_address, n, on_host, op, stream) -> 0 on success: in-place all-reduce of n doubles (device buffer = d_buf, or a
        host address); op 0 sum, 1 max."""
        self._ar_cb = self.ALLREDUCE_FN(lambda ctx, buf, n, on_host, op, stream: int(fn(buf, n, on_host, op, stream)))
        f = self.L.dvm_ba_set_allreduce
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.h, self._ar_cb, None, C.c_void_p(d_buf), C.c_int64(cap_doubles)))

    def optimize(self, iterations, stop_flag=None):
        st = BaStats()
        check(self.L.dvm_ba_optimize(self.h, iterations, _p(stop_flag) if stop_flag is not None else None, C.byref(st)))
        n = min(st.iterations, 64)
        return dict(iterations=st.iterations, total_trials=st.total_trials, stop_reason=st.stop_reason,
                    chi2_initial=st.chi2_initial, chi2_final=st.chi2_final, lambda_final=st.lambda_final,
                    trials=st.trials_per_iter[:n], chi2=st.chi2_per_iter[:n], lam=st.lambda_per_iter[:n],   # (a ctypes array slice is a list)
                    ms_structure=st.ms_structure, ms_optimize=st.ms_optimize, spec_trials=st.spec_trials, spec_kept=st.spec_kept)

    def set_edge_flags(self, flags):
        """dvm_ba_set_edge_flags: per edge BA_EDGE_ACTIVE | BA_EDGE_ROBUST (None: every edge active and robust again)."""
        f = self.L.dvm_ba_set_edge_flags
        f.restype = C.c_int32; f.argtypes = None
        if flags is None:
            check(f(self.h, None))
        else:
            fl = np.ascontiguousarray(flags, np.uint8)
            assert len(fl) == self.E
            check(f(self.h, _p(fl)))

    def result(self):
        poses = np.zeros((self.P, 7), np.float64)
        points = np.zeros((self.Lm, 3), np.float64)
        check(self.L.dvm_ba_get_result(self.h, _p(poses), _p(points)))
        return poses, points

    def edge_chi2(self):
        chi = np.zeros(self.E, np.float64)
        dp = np.zeros(self.E, np.uint8)
        check(self.L.dvm_ba_edge_chi2(self.h, _p(chi), _p(dp)))
        return chi, dp


class BaWindow(C.Structure):
    """dvm_ba_window (include/dvmslam_hip.h)"""
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32), ("iterations", C.c_int32),
                ("poses", C.c_void_p), ("fixed", C.c_void_p), ("points", C.c_void_p), ("edges", C.c_void_p), ("cam", BaCamera),
                ("poses_out", C.c_void_p), ("points_out", C.c_void_p), ("edge_chi2_out", C.c_void_p), ("depth_positive_out", C.c_void_p)]


def ba_optimize_batch(problems, device=0, threads=0, stop_flag=None):
    """dvm_ba_optimize_batch: the same K problems, each on the general solver, up to `threads` of them concurrently (0: the library's default).
    Same arguments and return value as ba_optimize_windows."""
    return ba_optimize_windows(problems, device, stop_flag, _threads=int(threads), _batch=True)


class BaWindowBatch:
    """K bundle-adjustment windows marshalled ONCE into the dvm_ba_window array of the C ABI (input arrays referenced, output arrays allocated):
    what a C++ agent node holds anyway.  run() is then the bare library call -- the per-call Python work of ba_optimize_windows (~35 us per
    window) stays out of a timed loop.  A problem may carry `model` (a CameraModel) instead of, or beside, `intrinsics`: run(fast=True) then
    is dvm_ba_optimize_windows_fast_cam, with a window that has no model as the pinhole model of its intrinsics (rounded to float)."""

    def __init__(self, problems):
        K = len(problems)
        self.K = K
        self.wins = (BaWindow * max(K, 1))()
        self.stats = (BaStats * max(K, 1))()
        self.models = None      # the dvm_camera_model array, when any window has a model
        if any(pr.get("model") is not None for pr in problems):
            self.models = (CameraModel * max(K, 1))()
            for k, pr in enumerate(problems):
                m = pr.get("model")
                if m is None:
                    m = CameraModel.pinhole(*[float(v) for v in pr["intrinsics"]])
                assert isinstance(m, CameraModel)
                self.models[k] = m
        self.keep, self.outs = [], []
        for k, pr in enumerate(problems):
            poses = np.ascontiguousarray(pr["poses"], np.float64); points = np.ascontiguousarray(pr["points"], np.float64)
            fixed = np.ascontiguousarray(pr["fixed"], np.uint8); edges = np.ascontiguousarray(pr["edges"], BA_EDGE_DTYPE)
            o = dict(poses=np.zeros_like(poses), points=np.zeros_like(points), edge_chi2=np.zeros(len(edges), np.float64),
                     depth_positive=np.zeros(len(edges), np.uint8))
            self.keep.append((poses, points, fixed, edges)); self.outs.append(o)
            w = self.wins[k]
            w.n_poses, w.n_points, w.n_edges, w.iterations = len(poses), len(points), len(edges), int(pr["iterations"])
            w.poses, w.fixed, w.points, w.edges = poses.ctypes.data, fixed.ctypes.data, points.ctypes.data, edges.ctypes.data
            intr = pr["intrinsics"] if pr.get("model") is None else list(pr["model"].p[:4])   # (under a model cam's fx, fy, cx, cy are not what counts)
            w.cam = BaCamera(*[float(v) for v in intr], float(pr["huber_delta"]))
            w.poses_out, w.points_out, w.edge_chi2_out, w.depth_positive_out = (o["poses"].ctypes.data, o["points"].ctypes.data, o["edge_chi2"].ctypes.data,
                                                                                o["depth_positive"].ctypes.data)

    def run(self, device=0, stop_flag=None, fast=False, _threads=0, _batch=False, collect=True):
        """One library call over the K windows; returns the per-window dicts (the output arrays are this object's: copy what must outlive the next run).
        collect=False: the bare call -- results() builds the dicts (ctypes slices of the statistics: ~5 us a window) when they are wanted."""
        sf = _p(stop_flag) if stop_flag is not None else None
        if self.models is not None:
            if _batch or not fast:
                raise ValueError("a window with a camera model runs through run(fast=True) only: dvm_ba_optimize_windows and dvm_ba_optimize_batch are pinhole-only")
            f = lib().dvm_ba_optimize_windows_fast_cam
            f.restype = C.c_int32; f.argtypes = None
            check(f(C.c_int32(device), self.wins, self.models, C.c_int32(self.K), sf, self.stats))
        elif _batch:
            f = lib().dvm_ba_optimize_batch
            f.restype = C.c_int32; f.argtypes = None
            check(f(C.c_int32(device), self.wins, C.c_int32(self.K), C.c_int32(_threads), sf, self.stats))
        else:
            f = lib().dvm_ba_optimize_windows_fast if fast else lib().dvm_ba_optimize_windows
            f.restype = C.c_int32; f.argtypes = None
            check(f(C.c_int32(device), self.wins, C.c_int32(self.K), sf, self.stats))
        return self.results() if collect else None

    def results(self):
        for k, o in enumerate(self.outs):
            st = self.stats[k]
            n = min(st.iterations, 64)
            o["stats"] = dict(iterations=st.iterations, total_trials=st.total_trials, stop_reason=st.stop_reason, chi2_initial=st.chi2_initial,
                              chi2_final=st.chi2_final, lambda_final=st.lambda_final, trials=st.trials_per_iter[:n], chi2=st.chi2_per_iter[:n],
                              lam=st.lambda_per_iter[:n], ms_structure=st.ms_structure, ms_optimize=st.ms_optimize, kernel_us=st.kernel_us)
        return self.outs


class BaPool:
    """dvm_ba_pool_*: blocking one-window calls from any number of threads, batched behind the boundary into launches of the cluster form."""

    def __init__(self, device=0, max_batch=32, window_us=-1):
        self.p = C.c_void_p()
        f = lib().dvm_ba_pool_create
        f.restype = C.c_int32; f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
        check(f(device, max_batch, window_us, C.byref(self.p)))

    def close(self):
        if getattr(self, "p", None) and self.p.value:
            f = lib().dvm_ba_pool_destroy
            f.restype = None; f.argtypes = [C.c_void_p]
            f(self.p)
            self.p = C.c_void_p()

    __del__ = close

    def optimize(self, batch: "BaWindowBatch"):
        """batch: a BaWindowBatch of ONE window (marshalled by the caller's thread).  Returns (result dict, windows in the launch)."""
        n = C.c_int32(0)
        if batch.models is not None:      # the window has a model: dvm_ba_pool_optimize_cam
            f = lib().dvm_ba_pool_optimize_cam
            f.restype = C.c_int32; f.argtypes = None
            check(f(self.p, batch.wins, batch.models, batch.stats, C.byref(n)))
            return batch.results()[0], n.value
        f = lib().dvm_ba_pool_optimize
        f.restype = C.c_int32; f.argtypes = None
        check(f(self.p, batch.wins, batch.stats, C.byref(n)))
        return batch.results()[0], n.value


def ba_optimize_windows(problems, device=0, stop_flag=None, _threads=0, _batch=False, fast=False):
    """dvm_ba_optimize_windows: K independent bundle adjustments in one launch.  problems: dicts with poses [P,7], fixed [P], points [L,3],
    edges (BA_EDGE_DTYPE), intrinsics (fx, fy, cx, cy) or model (a CameraModel: fast=True only, see BaWindowBatch), huber_delta, iterations.  Returns one dict per window: poses, points, edge_chi2,
    depth_positive, stats (the keys of BundleAdjuster.optimize).  fast=True: dvm_ba_optimize_windows_fast (tree sums in a fixed order)."""
    return BaWindowBatch(problems).run(device, stop_flag, fast, _threads, _batch)


def f64_spec_eval(x, device=0):
    """csrc/f64_spec.h on the device: returns (sin, cos, cube) of the doubles in x."""
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros(3 * len(x), np.float64)
    f = lib().dvm_f64_spec_eval
    f.restype = C.c_int32; f.argtypes = None
    check(f(C.c_int32(device), _p(x), C.c_int32(len(x)), _p(out)))
    return out[:len(x)], out[len(x):2 * len(x)], out[2 * len(x):]


def pose_optimize(poses, Xw, obs, inv_sigma2, n, intrinsics, device=0):
    """Optimizer::PoseOptimization for a batch of frames.  poses [B,7]; Xw [B,S,3]; obs [B,S,2]; inv_sigma2 [B,S];
    n [B].  Returns (poses [B,7], outlier [B,S] uint8, n_inliers [B])."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
    B = len(poses)
    Xw = np.ascontiguousarray(Xw, np.float64).reshape(B, -1, 3)
    S = Xw.shape[1]
    obs = np.ascontiguousarray(obs, np.float64).reshape(B, S, 2)
    inv_sigma2 = np.ascontiguousarray(inv_sigma2, np.float64).reshape(B, S)
    n = np.ascontiguousarray(n, np.int32).reshape(B)
    cam = BaCamera(*[float(v) for v in intrinsics], 0.0)
    out = np.zeros((B, 7), np.float64)
    outl = np.zeros((B, S), np.uint8)
    nin = np.zeros(B, np.int32)
    check(lib().dvm_pose_optimize(device, _p(poses), _p(Xw), _p(obs), _p(inv_sigma2), _p(n), S, B, C.byref(cam), _p(out),
                                  _p(outl), _p(nin)))
    return out, outl, nin


def pose_optimize_cam(poses, Xw, obs, inv_sigma2, n, model, device=0):
    """dvm_pose_optimize_cam: pose_optimize on a CameraModel (model 0: the pinhole kernel on its four floats)."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
    B = len(poses)
    Xw = np.ascontiguousarray(Xw, np.float64).reshape(B, -1, 3)
    S = Xw.shape[1]
    obs = np.ascontiguousarray(obs, np.float64).reshape(B, S, 2)
    inv_sigma2 = np.ascontiguousarray(inv_sigma2, np.float64).reshape(B, S)
    n = np.ascontiguousarray(n, np.int32).reshape(B)
    out = np.zeros((B, 7), np.float64)
    outl = np.zeros((B, S), np.uint8)
    nin = np.zeros(B, np.int32)
    fn = lib().dvm_pose_optimize_cam
    fn.restype = C.c_int32; fn.argtypes = None
    check(fn(C.c_int32(device), _p(poses), _p(Xw), _p(obs), _p(inv_sigma2), _p(n), C.c_int32(S), C.c_int32(B), None if model is None else C.byref(model),
             _p(out), _p(outl), _p(nin)))
    return out, outl, nin


def is_in_frustum_cam(F: "FrustumFrame", model, P, normal, min_dist, max_dist, viewing_cos_limit=0.5):
    """dvm_is_in_frustum_cam: is_in_frustum with the projection of a CameraModel (F.fx, fy, cx, cy are not read)."""
    P = np.ascontiguousarray(P, np.float32); normal = np.ascontiguousarray(normal, np.float32)
    min_dist = np.ascontiguousarray(min_dist, np.float32); max_dist = np.ascontiguousarray(max_dist, np.float32)
    out = np.zeros(len(P), TRACK_DTYPE)
    fn = lib().dvm_is_in_frustum_cam
    fn.restype = C.c_int32; fn.argtypes = None
    check(fn(C.byref(F), None if model is None else C.byref(model), _p(P), _p(normal), _p(min_dist), _p(max_dist), C.c_int32(len(P)),
             C.c_float(float(viewing_cos_limit)), _p(out), C.c_int32(0), None))
    return out


def is_in_frustum(F: "FrustumFrame", P, normal, min_dist, max_dist, viewing_cos_limit=0.5):
    """Frame::isInFrustum for an array of map points; returns a TRACK_DTYPE array."""
    P = np.ascontiguousarray(P, np.float32); normal = np.ascontiguousarray(normal, np.float32)
    min_dist = np.ascontiguousarray(min_dist, np.float32); max_dist = np.ascontiguousarray(max_dist, np.float32)
    out = np.zeros(len(P), TRACK_DTYPE)
    check(lib().dvm_is_in_frustum(C.byref(F), _p(P), _p(normal), _p(min_dist), _p(max_dist), len(P), float(viewing_cos_limit),
                                  _p(out), 0, None))
    return out


def triangulate_matches(K1, K2, T1w, T2w, Ow1, Ow2, kps1, kps2, pairs, sigma2_1, sigma2_2, sf1, sf2, ratio_factor,
                        cos_parallax_max=0.9998, far_points=False, th_far=0.0):
    """LocalMapping::CreateNewMapPoints' per-match geometry for one neighbour keyframe (dvm_triangulate_matches).
    Returns (x3D[n,3] float32, status[n] int32)."""
    P = TriPair()
    P.cos_parallax_max = float(cos_parallax_max)
    for name, v, k in (("K1", K1, 4), ("K2", K2, 4), ("T1w", T1w, 12), ("T2w", T2w, 12), ("Ow1", Ow1, 3), ("Ow2", Ow2, 3)):
        setattr(P, name, (C.c_float * k)(*np.asarray(v, np.float32).reshape(-1)))
    f = [np.ascontiguousarray(x, np.float32) for x in (sigma2_1, sigma2_2, sf1, sf2)]
    P.ratio_factor = float(ratio_factor); P.th_far = float(th_far); P.far_points = int(far_points); P.n_levels = len(f[0])
    k1 = np.ascontiguousarray(kps1); k2 = np.ascontiguousarray(kps2)
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n = len(pr)
    X = np.zeros((n, 3), np.float32); st = np.zeros(n, np.int32)
    L = lib()
    L.dvm_triangulate_matches.restype = C.c_int
    L.dvm_triangulate_matches.argtypes = [C.POINTER(TriPair), C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    check(L.dvm_triangulate_matches(C.byref(P), _p(k1), len(k1), _p(k2), len(k2), _p(pr), n, _p(f[0]), _p(f[1]), _p(f[2]), _p(f[3]), _p(X), _p(st), 0, None))
    return X, st


class PairPose(C.Structure):   # == dvm_pair_pose
    """The relative pose of a keyframe pair (R12, t12 of T12 = T1w * Tw2) and R21 = R12^T, t21 = -R21 t12 (dvm_pair_pose_set)."""
    _fields_ = [("R12", C.c_float * 9), ("t12", C.c_float * 3), ("R21", C.c_float * 9), ("t21", C.c_float * 3)]


def pair_pose(R12, t12):
    R12 = np.ascontiguousarray(R12, np.float32).reshape(9); t12 = np.ascontiguousarray(t12, np.float32).reshape(3)
    out = PairPose()
    fn = lib().dvm_pair_pose_set
    fn.restype = None; fn.argtypes = None
    fn(_p(R12), _p(t12), C.byref(out))
    return out


def _model_ref(m):
    return None if m is None else C.byref(m)


def triangulate_matches_cam(model1, model2, T1w, T2w, Ow1, Ow2, kps1, kps2, pairs, sigma2_1, sigma2_2, sf1, sf2, ratio_factor,
                            cos_parallax_max=0.9998, far_points=False, th_far=0.0):
    """dvm_triangulate_matches_cam: triangulate_matches with the rays and both reprojections through a CameraModel per keyframe (both of
    one model type).  Returns (x3D[n,3] float32, status[n] int32)."""
    P = TriPair()
    P.cos_parallax_max = float(cos_parallax_max)
    for name, v, k in (("T1w", T1w, 12), ("T2w", T2w, 12), ("Ow1", Ow1, 3), ("Ow2", Ow2, 3)):
        setattr(P, name, (C.c_float * k)(*np.asarray(v, np.float32).reshape(-1)))
    f = [np.ascontiguousarray(x, np.float32) for x in (sigma2_1, sigma2_2, sf1, sf2)]
    P.ratio_factor = float(ratio_factor); P.th_far = float(th_far); P.far_points = int(far_points); P.n_levels = len(f[0])
    k1 = np.ascontiguousarray(kps1); k2 = np.ascontiguousarray(kps2)
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n = len(pr)
    X = np.zeros((n, 3), np.float32); st = np.zeros(n, np.int32)
    fn = lib().dvm_triangulate_matches_cam
    fn.restype = C.c_int32; fn.argtypes = None
    check(fn(C.byref(P), _model_ref(model1), _model_ref(model2), _p(k1), C.c_int32(len(k1)), _p(k2), C.c_int32(len(k2)), _p(pr), C.c_int32(n), _p(f[0]), _p(f[1]),
             _p(f[2]), _p(f[3]), _p(X), _p(st), C.c_int32(0), None))
    return X, st


def match_triangulation_cam(desc1, kps1, qidx, desc2, kps2, off, cand, model1, model2, pose, ep, coarse, level_sigma2_1, scale_factors2,
                            level_sigma2_2, F12=None):
    """dvm_match_triangulation_cam: SearchForTriangulation's inner loop on a CameraModel per keyframe.  Query q = keypoint qidx[q] of KF1
    scans cand[off[q] .. off[q+1]).  pose: a PairPose (read under KannalaBrandt8), F12: read under model 0.  Returns (best_idx, best_dist)."""
    d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
    k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
    qi = np.ascontiguousarray(qidx, np.int32); of = np.ascontiguousarray(off, np.int32)
    cd = np.ascontiguousarray(cand, np.int32)
    if cd.size == 0:
        cd = np.full(1, -1, np.int32)
    epf = np.ascontiguousarray(ep, np.float32)
    s1 = np.ascontiguousarray(level_sigma2_1, np.float32); sf2 = np.ascontiguousarray(scale_factors2, np.float32); s2 = np.ascontiguousarray(level_sigma2_2, np.float32)
    F = None if F12 is None else np.ascontiguousarray(F12, np.float32)
    nq = len(qi)
    bi = np.zeros(max(nq, 1), np.int32); bd = np.zeros(max(nq, 1), np.int32)
    fn = lib().dvm_match_triangulation_cam
    fn.restype = C.c_int32; fn.argtypes = None
    check(fn(_p(d1), _p(k1), C.c_int32(len(k1)), _p(qi), C.c_int32(nq), _p(d2), _p(k2), C.c_int32(len(k2)), _p(of), _p(cd), _model_ref(model1), _model_ref(model2),
             None if pose is None else C.byref(pose), None if F is None else _p(F), _p(epf), C.c_int32(int(coarse)), _p(s1), _p(sf2), _p(s2), C.c_int32(len(s2)),
             _p(bi), _p(bd), C.c_int32(0), None))
    return bi[:nq], bd[:nq]


def undistort_keypoints(cam, kps, d_in=None, d_out=None, n=None, stream=None):
    """Frame::UndistortKeyPoints: cam = (fx, fy, cx, cy, k1, k2, p1, p2, k3) float32; kps a KP_DTYPE array (returns the
    undistorted copy), or device pointers d_in / d_out of n keypoints (asynchronous on `stream`)."""
    cam = np.ascontiguousarray(cam, np.float32)
    assert cam.shape == (9,)
    if d_in is not None:
        check(lib().dvm_undistort_keypoints(_p(cam), d_in, d_out, int(n), 1, stream))
        return None
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    out = np.zeros_like(kps)
    check(lib().dvm_undistort_keypoints(_p(cam), _p(kps), _p(out), len(kps), 0, None))
    return out


def image_bounds(cam, cols, rows):
    """Frame::ComputeImageBounds -> float32 (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    cam = np.ascontiguousarray(cam, np.float32)
    out = np.zeros(4, np.float32)
    check(lib().dvm_image_bounds(_p(cam), int(cols), int(rows), _p(out)))
    return out


def optimize_sim3(S12, fix_scale, P1c, P2c, obs1, obs2, w1, w2, K1, K2, th2, device=0):
    """Optimizer::OptimizeSim3 numerics on the device.  Returns (S12[8], inlier mask, nIn)."""
    S = np.array(S12, np.float64, copy=True)
    arrs = [np.ascontiguousarray(a, np.float64) for a in (P1c, P2c, obs1, obs2, w1, w2, K1, K2)]
    n = len(arrs[0])
    inl = np.zeros(n, np.uint8)
    nin = C.c_int32(0)
    check(lib().dvm_optimize_sim3(device, _p(S), int(fix_scale), *[_p(a) for a in arrs[:6]], n, _p(arrs[6]), _p(arrs[7]),
                                  float(th2), _p(inl), C.byref(nin)))
    return S, inl, nin.value


def optimize_sim3_cam(S12, fix_scale, P1c, P2c, obs1, obs2, w1, w2, model1, model2, th2, device=0):
    """dvm_optimize_sim3_cam: OptimizeSim3 with a CameraModel per keyframe (any pair of pinhole / KannalaBrandt8).  On a KannalaBrandt8
    side the residual and the chi2 tests use the reference's project(Vector3d) (float theta), the numeric Jacobian the projection with the
    double atan2.  Returns (S12[8], inlier mask, nIn); two pinhole models give optimize_sim3's outputs bit for bit."""
    L = lib()
    vp, i32 = C.c_void_p, C.c_int32
    L.dvm_optimize_sim3_cam.restype = i32
    L.dvm_optimize_sim3_cam.argtypes = [i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, C.c_double, vp, vp]
    S = np.array(S12, np.float64, copy=True)
    arrs = [np.ascontiguousarray(a, np.float64) for a in (P1c, P2c, obs1, obs2, w1, w2)]
    n = len(arrs[0])
    inl = np.zeros(n, np.uint8)
    nin = C.c_int32(0)
    check(L.dvm_optimize_sim3_cam(device, _p(S), int(fix_scale), *[_p(a) for a in arrs], n, C.addressof(model1), C.addressof(model2),
                                  float(th2), _p(inl), C.addressof(nin)))
    return S, inl, nin.value


# ---- host C++ mirror (dvm_slam_amd/host, libdvmslam_host.so): ORBmatcher on plain structs over the C ABI
HOST_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libdvmslam_host.so")
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("desc", "u1", (32,)), ("n_obs", "<i4")])
_HOST = None


def host_lib():
    global _HOST
    if _HOST is None:
        lib()  # HIP library (and torch's runtime) first
        if not os.path.exists(HOST_LIB_PATH):
            raise ImportError(f"{HOST_LIB_PATH} not built (make -C dvm_slam_amd/host)")
        _HOST = C.CDLL(HOST_LIB_PATH)
        vp = C.c_void_p
        _HOST.dvmh_search_by_projection_frames.restype = C.c_int32
        _HOST.dvmh_search_by_projection_frames.argtypes = [C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, C.c_int32,
                                                           C.c_int32, vp, vp, vp, vp, C.c_float, C.c_int32, vp]
        _declare(_HOST, _TRACK_HOST_API)
    return _HOST


class DeviceFrame(C.Structure):
    """dvm_device_frame (include/dvmslam_hip.h): the extractor's last single-frame result, still in HBM"""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("n", C.c_int32), ("device", C.c_int32), ("handle_id", C.c_uint64), ("serial", C.c_uint64)]


def search_by_projection_frames(kps_c, desc_c, mp_c, Tcw, K, bounds, scale_factors, kps_l, mp_l, outlier_l, mps, th,
                                check_ori=True, device=0, dev_c=None):
    """dvm_host::ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono=true) -- reference
    ORBmatcher.cc:1553-1748.  Tcw: CurrentFrame.GetPose() as 7 floats (qx, qy, qz, qw, t).  Returns (nmatches, updated mvpMapPoints of the current frame, #host re-queries)."""
    H = host_lib()
    kps_c = np.ascontiguousarray(kps_c, KP_DTYPE); kps_l = np.ascontiguousarray(kps_l, KP_DTYPE)
    desc_c = np.ascontiguousarray(desc_c, np.uint8)
    mp = np.array(mp_c, np.int32, copy=True)
    mp_l = np.ascontiguousarray(mp_l, np.int32)
    outl = None if outlier_l is None else np.ascontiguousarray(outlier_l, np.uint8)
    f = [np.ascontiguousarray(a, np.float32) for a in (Tcw, K, bounds, scale_factors)]
    assert f[0].shape == (7,)
    mps = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
    req = C.c_int32(0)
    if dev_c is not None:       # the current frame's data is still in HBM (OrbExtractor.last_result()): returns a 4th value, 1 if the grid was built from it
        fn = H.dvmh_search_by_projection_frames_dev
        fn.restype = C.c_int32; fn.argtypes = None
        used = C.c_int32(0)
        n = fn(C.c_int32(device), C.c_int32(len(kps_c)), _p(kps_c), _p(desc_c), _p(mp), *[_p(a) for a in f], C.c_int32(len(f[3])), C.c_int32(len(kps_l)), _p(kps_l),
               _p(mp_l), None if outl is None else _p(outl), _p(mps), C.c_float(float(th)), C.c_int32(int(check_ori)), C.byref(req), C.byref(dev_c), C.byref(used))
        if n < 0:
            check(n)
        return n, mp, req.value, used.value
    n = H.dvmh_search_by_projection_frames(device, len(kps_c), _p(kps_c), _p(desc_c), _p(mp), *[_p(a) for a in f],
                                           len(f[3]), len(kps_l), _p(kps_l), _p(mp_l), None if outl is None else _p(outl),
                                           _p(mps), float(th), int(check_ori), C.byref(req))
    if n < 0:
        check(n)
    return n, mp, req.value


def search_by_projection_frames_cam(kps_c, desc_c, mp_c, Tcw, model, bounds, scale_factors, kps_l, mp_l, outlier_l, mps, th,
                                    check_ori=True, device=0):
    """dvmh_search_by_projection_frames_cam: search_by_projection_frames with the query projection of a CameraModel in place of K.
    Returns (nmatches, updated mvpMapPoints of the current frame, #host re-queries)."""
    H = host_lib()
    kps_c = np.ascontiguousarray(kps_c, KP_DTYPE); kps_l = np.ascontiguousarray(kps_l, KP_DTYPE)
    desc_c = np.ascontiguousarray(desc_c, np.uint8)
    mp = np.array(mp_c, np.int32, copy=True)
    mp_l = np.ascontiguousarray(mp_l, np.int32)
    outl = None if outlier_l is None else np.ascontiguousarray(outlier_l, np.uint8)
    T, b, sf = [np.ascontiguousarray(a, np.float32) for a in (Tcw, bounds, scale_factors)]
    assert T.shape == (7,)
    mps = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
    req = C.c_int32(0)
    fn = H.dvmh_search_by_projection_frames_cam
    fn.restype = C.c_int32; fn.argtypes = None
    n = fn(C.c_int32(device), C.c_int32(len(kps_c)), _p(kps_c), _p(desc_c), _p(mp), _p(T), None if model is None else C.byref(model), _p(b), _p(sf),
           C.c_int32(len(sf)), C.c_int32(len(kps_l)), _p(kps_l), _p(mp_l), None if outl is None else _p(outl), _p(mps), C.c_float(float(th)),
           C.c_int32(int(check_ori)), C.byref(req))
    if n < 0:
        check(n)
    return n, mp, req.value


class TrackResult(C.Structure):
    """dvmh_track_result (include/dvmslam_host.h)"""
    _fields_ = [("n", C.c_int32), ("mono_index", C.c_int32), ("nmatches", C.c_int32), ("nmatches_search", C.c_int32), ("nmatches_map", C.c_int32),
                ("n_inliers", C.c_int32), ("wide_window", C.c_int32), ("replayed_on_host", C.c_int32), ("tracked", C.c_int32),
                ("Tcw", C.c_float * 7), ("pose", C.c_double * 7), ("n_requeried", C.c_int32), ("pad_", C.c_int32)]


class Distortion(C.Structure):
    """dvm_distortion (include/dvmslam_hip.h)"""
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


# dvm_local_point (include/dvmslam_hip.h): one mvpLocalMapPoints entry -- GetWorldPos, GetNormal, mfMinDistance / mfMaxDistance,
# GetDescriptor, Observations, isBad
LOCAL_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_dist", "<f4"), ("max_dist", "<f4"), ("desc", "u1", (32,)),
                              ("n_obs", "<i4"), ("bad", "<i4")])


class TrackLocalResult(C.Structure):
    """dvm_track_local_result (include/dvmslam_hip.h)"""
    _fields_ = [(k, C.c_int32) for k in ("n_to_match", "nmatches", "n_requeried", "n_cleared_bad", "n_edges", "n_inliers", "matches_inliers",
                                         "reserved")] + [("pose", C.c_double * 7), ("Tcw", C.c_float * 7), ("reserved2", C.c_int32)]


# dvm_track_refkf_* (include/dvmslam_hip.h): the reference-keyframe chain's keyframe, parameters, outputs and result; DVM_TRACK_* statuses
DVM_TRACK_COMPLETE, DVM_TRACK_FEW_MATCHES, DVM_TRACK_FEW_MAP_MATCHES = 0, 1, 3


class RefKeyframe(C.Structure):
    """dvm_ref_keyframe (include/dvmslam_hip.h)"""
    _fields_ = [("n", C.c_int32), ("kps_un", C.c_void_p), ("desc", C.c_void_p), ("mp", C.c_void_p), ("mp_pos", C.c_void_p), ("mp_nobs", C.c_void_p),
                ("mp_bad", C.c_void_p), ("fv_n", C.c_int32), ("fv_node", C.c_void_p), ("fv_off", C.c_void_p), ("fv_feat", C.c_void_p)]


class TrackRefKfParams(C.Structure):
    """dvm_track_refkf_params (include/dvmslam_hip.h)"""
    _fields_ = [("pose_in", C.c_double * 7), ("nnratio", C.c_float), ("check_ori", C.c_int32), ("th_low", C.c_int32), ("min_matches", C.c_int32),
                ("min_map", C.c_int32), ("levelsup", C.c_int32), ("bounds", C.c_float * 4), ("dist", C.c_void_p), ("inv_level_sigma2", C.c_void_p),
                ("nlevels", C.c_int32), ("cam", BaCamera)]


class TrackRefKfOut(C.Structure):
    """dvm_track_refkf_out (include/dvmslam_hip.h)"""
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("cap", C.c_int32), ("kps_un", C.c_void_p), ("mp_out", C.c_void_p), ("dropped", C.c_void_p),
                ("outlier", C.c_void_p), ("bow_ids", C.c_void_p), ("bow_vals", C.c_void_p), ("fv_node", C.c_void_p), ("fv_off", C.c_void_p),
                ("fv_feat", C.c_void_p)]


class TrackRefKfResult(C.Structure):
    """dvm_track_refkf_result (include/dvmslam_hip.h)"""
    _fields_ = [(k, C.c_int32) for k in ("n", "mono_index", "status", "nmatches", "nmatches_before_rotation", "n_edges", "n_inliers",
                                         "nmatches_after", "nmatches_map", "n_bow", "n_fv", "reserved")] + \
               [("pose", C.c_double * 7), ("Tcw", C.c_float * 7), ("reserved2", C.c_int32)]


class TrackIn(C.Structure):
    """dvmh_track_in (include/dvmslam_host.h); dvmh_track_in_resident has the same layout: the store's handle where mps is"""
    _fields_ = [("Tcw_pred", C.c_void_p), ("Nl", C.c_int32), ("kps_l", C.c_void_p), ("mp_l", C.c_void_p), ("outlier_l", C.c_void_p), ("mps", C.c_void_p)]


class TrackOut(C.Structure):
    """dvmh_track_out (include/dvmslam_host.h)"""
    _fields_ = [("kps", C.c_void_p), ("desc", C.c_void_p), ("cap", C.c_int32), ("kps_un", C.c_void_p), ("mp_c", C.c_void_p), ("dropped", C.c_void_p)]


class LocalMapIn(C.Structure):
    """dvm_local_map_in (include/dvmslam_hip.h)"""
    _fields_ = [("pts", C.c_void_p), ("n", C.c_int32), ("frame_mp", C.c_void_p), ("th", C.c_float), ("far_points", C.c_int32), ("th_far", C.c_float)]


class LocalMapOut(C.Structure):
    """dvm_local_map_out (include/dvmslam_hip.h)"""
    _fields_ = [("mp_out", C.c_void_p), ("outlier", C.c_void_p), ("track_pts", C.c_void_p)]


class TrackLast(C.Structure):
    """dvm_track_last (include/dvmslam_hip.h)"""
    _fields_ = [("store", C.c_void_p), ("n", C.c_int32), ("slot", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p),
                ("Tcw_pred", C.c_float * 7), ("th", C.c_float)]


class TrackShared(C.Structure):
    """dvm_track_shared (include/dvmslam_hip.h)"""
    _fields_ = [("bounds", C.c_float * 4), ("dist", C.c_void_p), ("scale_factors", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("nlevels", C.c_int32),
                ("cam", BaCamera), ("th_high", C.c_int32), ("check_ori", C.c_int32), ("min_matches", C.c_int32)]


class LocalMapInResident(C.Structure):
    """dvm_local_map_in_resident (include/dvmslam_hip.h)"""
    _fields_ = [("store", C.c_void_p), ("slots", C.c_void_p), ("n", C.c_int32), ("frame_mp", C.c_void_p), ("th", C.c_float), ("far_points", C.c_int32),
                ("th_far", C.c_float)]


# ---- the tracker entry points of both libraries, declared once: name -> argument types (restype int32 but for the destroy).  lib() and
# host_lib() apply the tables when they load their library, so a call with a wrong count or a float where an int belongs raises.  No more
# than that: pointers are not told apart (two of them swapped pass), an array's dtype is not looked at.
class _Ptr:
    """The argtype of a pointer argument: None, a C-contiguous numpy array (its data), a ctypes structure or array (its address), an
    address, or what ctypes takes as a pointer anyway (c_void_p, byref(), pointer())."""

    @classmethod
    def from_param(cls, v):
        if isinstance(v, np.ndarray):
            if not v.flags.c_contiguous:
                raise TypeError("a numpy array passed to the C ABI must be C-contiguous")
            return C.c_void_p(v.ctypes.data)
        if isinstance(v, (C.Structure, C.Array)):
            return C.byref(v)
        if isinstance(v, int) and not isinstance(v, bool):
            return C.c_void_p(v)
        return v


_I, _L, _F, _P = C.c_int32, C.c_int64, C.c_float, _Ptr
_TRACK_ONE = [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _F, _I, _P, _P, _I, _P, _P, _P, _P]
_TRACK_BATCH = [_P, _P, _I, _I, _P, _I, _I, _I, _L, _I, _I, _P, _P, _P, _P, _I, _F, _I, _P, _P, _P]
_TRACK_API = {            # libdvmslam_hip.so (include/dvmslam_hip.h)
    "dvm_tracker_create": [_I, _I, _I, _P],
    "dvm_tracker_create_batch": [_I, _I, _I, _I, _P],
    "dvm_tracker_destroy": [_P],
    "dvm_tracker_set_camera_model": [_P, _P],
    "dvm_tracker_last_upload_bytes": [_P, _P, _P],
    "dvm_tracker_reserve_local_map": [_P, _I],
    "dvm_tracker_reserve_reference_keyframe": [_P, _I],
    "dvm_tracker_reserve_reference_keyframe_batch": [_P, _I],
    "dvm_track_begin": [_P, _P, _P, _I, _I, _I, _I, _I],
    "dvm_track_begin_batch": [_P, _P, _P, _I, _I, _I, _I, _L, _I, _I],
    "dvm_track_begin_staged": [_P, _P, _I, _I, _I, _I, _I],
    "dvm_track_finish": [_P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P],
    "dvm_track_finish_batch": [_P, _P, _I, _P, _P, _P],
    "dvm_track_finish_batch_resident": [_P, _P, _I, _P, _P, _P, _P],
    "dvm_track_debug_build_queries": [_P, _I, _P, _P] + [_P] * 12,
    "dvm_track_local_map": [_P, _P, _P, _I, _P, _F, _I, _F, _P, _P, _P, _P],
    "dvm_track_local_map_batch": [_P, _P, _I, _P, _P, _P, _P],
    "dvm_track_local_map_batch_resident": [_P, _P, _I, _P, _P, _P, _P],
    "dvm_track_reference_keyframe": [_P] * 7,
    "dvm_track_reference_keyframe_batch": [_P, _P, _P, _I, _P, _P, _P, _P, _P],
    "dvm_track_reference_keyframe_batch_resident": [_P, _P, _P, _P, _I, _P, _P, _P, _P, _P],
    "dvm_tracker_last_refkf_upload_bytes": [_P, _P],
}
_TRACK_HOST_API = {       # libdvmslam_host.so (include/dvmslam_host.h); the _cam forms take the model behind K
    "dvmh_track_with_motion_model": _TRACK_ONE,
    "dvmh_track_with_motion_model_cam": _TRACK_ONE[:11] + [_P] + _TRACK_ONE[11:],
    "dvmh_track_with_motion_model_batch": _TRACK_BATCH,
    "dvmh_track_with_motion_model_batch_cam": _TRACK_BATCH[:12] + [_P] + _TRACK_BATCH[12:],
    "dvmh_track_with_motion_model_batch_resident": _TRACK_BATCH,
    "dvmh_build_frame_queries": [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _F] + [_P] * 10,
}


def _declare(L, api):
    for name, argtypes in api.items():
        f = getattr(L, name, None)
        if f is None:       # an older library (DVM_HIP_LIB, the measurement tools' baseline): calling the entry raises AttributeError
            continue
        f.restype = None if name.endswith("_destroy") else C.c_int32
        f.argtypes = argtypes


_TRACK_COUNTERS = ("n", "mono_index", "nmatches", "nmatches_search", "nmatches_map", "n_inliers", "wide_window", "replayed_on_host", "tracked", "n_requeried")
_LOCAL_COUNTERS = ("n_to_match", "nmatches", "n_requeried", "n_cleared_bad", "n_edges", "n_inliers", "matches_inliers")
_REFKF_COUNTERS = ("n", "mono_index", "status", "nmatches", "nmatches_before_rotation", "n_edges", "n_inliers", "nmatches_after", "nmatches_map", "n_bow", "n_fv")
_QUERY_ARRAYS = ("q_entry", "qx", "qy", "qr", "qmin", "qmax", "q_claims", "q_angle", "q_pos", "qdesc")


def _f32(*arrays):
    return [None if a is None else np.ascontiguousarray(a, np.float32) for a in arrays]


def _per_frame(v, count):
    return list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * count


def _need_K(K, model):
    if K is None:
        if model is None:
            raise ValueError("K is needed without a camera model")
        K = model.p[:4]
    return K


def _ref_keyframe(kf):
    """dvm_ref_keyframe of a keyframe dict (Tracker.track_reference_keyframe's kf); returns it and the arrays it points into."""
    keep = [np.ascontiguousarray(kf["kps"], KP_DTYPE), np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32), np.ascontiguousarray(kf["mp"], np.int32),
            np.ascontiguousarray(kf["pos"], np.float32).reshape(-1, 3), np.ascontiguousarray(kf["n_obs"], np.int32)]
    bad = None if kf.get("bad") is None else np.ascontiguousarray(kf["bad"], np.uint8)
    fv = [np.ascontiguousarray(kf["fv"][k], np.int32) for k in ("fv_nodes", "fv_off", "fv_feat")]
    rk = RefKeyframe()
    rk.n = len(keep[0])
    rk.kps_un, rk.desc, rk.mp, rk.mp_pos, rk.mp_nobs = (a.ctypes.data if len(a) else None for a in keep)
    rk.mp_bad = None if bad is None or not len(bad) else bad.ctypes.data
    rk.fv_n = len(fv[0])
    rk.fv_node, rk.fv_off, rk.fv_feat = (a.ctypes.data if len(a) else None for a in fv)
    return rk, (keep, bad, fv)


def _refkf_params(pose_last, K, inv_sigma2, nnratio, check_ori, th_low, min_matches, min_map, levelsup):
    """dvm_track_refkf_params (bounds zero, no distortion); returns it and the level table it points into."""
    T = np.asarray(pose_last, np.float32).reshape(7)
    pr = TrackRefKfParams()
    pr.pose_in[:] = [float(v) for v in np.concatenate([T[4:7], T[0:4]]).astype(np.float64)]
    pr.nnratio, pr.check_ori, pr.th_low, pr.min_matches, pr.min_map, pr.levelsup = float(nnratio), int(check_ori), int(th_low), int(min_matches), int(min_map), int(levelsup)
    s2 = np.ascontiguousarray(inv_sigma2, np.float32)
    pr.inv_level_sigma2, pr.nlevels = s2.ctypes.data, len(s2)
    Kf = np.asarray(K, np.float32)
    pr.cam = BaCamera(*[float(v) for v in Kf[:4]], 0.0)
    return pr, s2


def _refkf_out(cap):
    """dvm_track_refkf_out for a frame of up to cap keypoints (kps / desc / kps_un unset) and the arrays it points into."""
    arrs = dict(mp=np.empty(cap, np.int32), dropped=np.empty(cap, np.int32), outlier=np.empty(cap, np.uint8), bow_ids=np.empty(cap, np.int32),
                bow_vals=np.empty(cap, np.float64), fv_nodes=np.empty(cap, np.int32), fv_off=np.empty(cap + 1, np.int32), fv_feat=np.empty(cap, np.int32))
    o = TrackRefKfOut()
    o.mp_out, o.dropped, o.outlier = arrs["mp"].ctypes.data, arrs["dropped"].ctypes.data, arrs["outlier"].ctypes.data
    o.bow_ids, o.bow_vals = arrs["bow_ids"].ctypes.data, arrs["bow_vals"].ctypes.data
    o.fv_node, o.fv_off, o.fv_feat = arrs["fv_nodes"].ctypes.data, arrs["fv_off"].ctypes.data, arrs["fv_feat"].ctypes.data
    return o, arrs


def entry_lists(kps_l, mp_l, outlier_l=None):
    """LastFrame's entry lists as dvm_track_last takes them: the keypoints that hold a map point and are no outliers, in keypoint order.
    Returns (idx, slot, octave, angle): idx = the keypoint of every entry, slot = mp_l[idx]."""
    kps_l = np.ascontiguousarray(kps_l, KP_DTYPE); mp_l = np.ascontiguousarray(mp_l, np.int32)
    keep = mp_l >= 0
    if outlier_l is not None:
        keep &= np.asarray(outlier_l) == 0
    idx = np.nonzero(keep)[0].astype(np.int32)
    return idx, mp_l[idx].copy(), kps_l["octave"][idx].astype(np.uint8), kps_l["angle"][idx].astype(np.float32)


def _track_shared(K, bounds, scale_factors, inv_sigma2, check_ori=True, th_high=100, min_matches=20):
    sf = np.ascontiguousarray(scale_factors, np.float32); s2 = np.ascontiguousarray(inv_sigma2, np.float32)
    sh = TrackShared()
    sh.bounds[:] = [float(v) for v in np.asarray(bounds, np.float32)]
    sh.dist = None; sh.scale_factors = sf.ctypes.data; sh.inv_level_sigma2 = s2.ctypes.data; sh.nlevels = len(sf)
    if K is not None:
        sh.cam.fx, sh.cam.fy, sh.cam.cx, sh.cam.cy = [float(v) for v in np.asarray(K, np.float32)[:4]]
    sh.th_high, sh.check_ori, sh.min_matches = int(th_high), int(bool(check_ori)), int(min_matches)
    return sh, (sf, s2)


def _track_lasts(lasts):
    """lasts: per frame a dict(store (MapStore or None), slot, octave, angle, Tcw_pred (7 floats: q, t), th)"""
    arr = (TrackLast * len(lasts))()
    keep = []
    for b, d in enumerate(lasts):
        slot = np.ascontiguousarray(d["slot"], np.int32); octv = np.ascontiguousarray(d["octave"], np.uint8); ang = np.ascontiguousarray(d["angle"], np.float32)
        assert len(slot) == len(octv) == len(ang)
        keep.append((slot, octv, ang, d.get("store")))
        a = arr[b]
        a.store = None if d.get("store") is None else d["store"].h
        a.n = len(slot); a.slot = slot.ctypes.data; a.octave = octv.ctypes.data; a.angle = ang.ctypes.data
        a.Tcw_pred[:] = [float(v) for v in np.asarray(d["Tcw_pred"], np.float32)]
        a.th = float(d.get("th", 15.0))
    return arr, keep


def _query_arrays(m):
    """the ten per-query output arrays of the two query builders, m entries each"""
    return dict(q_entry=np.zeros(m, np.int32), qx=np.zeros(m, np.float32), qy=np.zeros(m, np.float32), qr=np.zeros(m, np.float32), qmin=np.zeros(m, np.int32),
                qmax=np.zeros(m, np.int32), q_claims=np.zeros(m, np.uint8), q_angle=np.zeros(m, np.float32), q_pos=np.zeros((m, 3), np.float32),
                qdesc=np.zeros((m, 32), np.uint8))


def build_frame_queries_host(last, K, bounds, scale_factors, records, model=None):
    """dvmh_build_frame_queries: the host's loop header of SearchByProjection(CurrentFrame, LastFrame) on one frame's entry lists, the map
    points given as `records` (LOCAL_POINT_DTYPE, indexed by last['slot']).  last: a dict as Tracker.debug_build_queries takes it (its
    store is not read).  Returns a dict: nq, q_entry, qx, qy, qr, qmin, qmax, q_claims, q_angle, q_pos [nq, 3], qdesc [nq, 32]."""
    slot = np.ascontiguousarray(last["slot"], np.int32); octv = np.ascontiguousarray(last["octave"], np.uint8); ang = np.ascontiguousarray(last["angle"], np.float32)
    records = np.ascontiguousarray(records, LOCAL_POINT_DTYPE)
    T, K4, b4, sf = _f32(last["Tcw_pred"], K, bounds, scale_factors)
    n = len(slot)
    o = _query_arrays(max(n, 1))
    nq = host_lib().dvmh_build_frame_queries(T, K4, model, b4, sf, len(sf), n, slot, records, octv, ang, float(last.get("th", 15.0)), *[o[k] for k in _QUERY_ARRAYS])
    if nq < 0:
        check(nq)
    out = {k: v[:nq] for k, v in o.items()}
    out["nq"] = nq
    return out


class _TrackerBase:
    """What Tracker and TrackerBatch share: the handle's life cycle, the reservations, the marshalling of a call's frames and the three
    result builders (first half, TrackLocalMap, TrackReferenceKeyFrame), each written once."""

    def _open(self, ext, device, max_frames, create, *sizes):
        self.L, self.H, self.ext, self.device, self.max_frames = lib(), host_lib(), ext, device, int(max_frames)
        self.t = C.c_void_p()
        check(create(device, *sizes, C.byref(self.t)))

    def close(self):
        if getattr(self, "t", None) and self.t.value:
            self.L.dvm_tracker_destroy(self.t)
            self.t = C.c_void_p()

    __del__ = close

    def set_camera_model(self, model):
        """dvm_tracker_set_camera_model: the camera of the agent this tracker serves, for every chain of the tracker.  model: a CameraModel, or
        None for the default (the pinhole K of each call).  Drops what the last begin / finish prepared for the second half."""
        check(self.L.dvm_tracker_set_camera_model(self.t, model))

    def reserve_local_map(self, n):
        """dvm_tracker_reserve_local_map: the second half's working set (allocated once) for tables of up to n points per call -- a batch:
        the sum over the frames of each table's size rounded up to 64; per-keypoint arrays for max_frames frames."""
        check(self.L.dvm_tracker_reserve_local_map(self.t, int(n)))

    def debug_build_queries(self, lasts, K, bounds, scale_factors, inv_sigma2):
        """dvm_track_debug_build_queries: k_track_queries alone.  lasts: per frame a dict(store, slot, octave, angle, Tcw_pred (7 floats: q, t),
        th).  Returns one dict per frame: nq, q_entry, qx, qy, qr, qmin, qmax, q_claims, q_angle, q_pos, qdesc."""
        count = len(lasts)
        arr, keep = _track_lasts(lasts)
        sh, keep2 = _track_shared(K, bounds, scale_factors, inv_sigma2)
        stride = max(64, (max(len(k[0]) for k in keep) + 63) & ~63)
        nq = np.zeros(count, np.int32)
        o = _query_arrays(count * stride)
        got = C.c_int32(0)
        check(self.L.dvm_track_debug_build_queries(self.t, count, arr, sh, nq, *[o[k] for k in _QUERY_ARRAYS], C.byref(got)))
        assert got.value == stride, (got.value, stride)
        out = []
        for b in range(count):
            d = {k: v[b * stride:b * stride + nq[b]].copy() for k, v in o.items()}
            d["nq"] = int(nq[b])
            out.append(d)
        return out

    def last_upload_bytes(self):
        """dvm_tracker_last_upload_bytes: (first half, second half) host-to-device bytes of the last finish and the last local-map call."""
        a, b = C.c_int64(0), C.c_int64(0)
        check(self.L.dvm_tracker_last_upload_bytes(self.t, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_refkf_upload_bytes(self):
        """dvm_tracker_last_refkf_upload_bytes: host-to-device bytes of the last reference-keyframe call that reached the device."""
        a = C.c_int64(0)
        check(self.L.dvm_tracker_last_refkf_upload_bytes(self.t, C.byref(a)))
        return a.value

    def _refkf_batch(self, voc, kfs, store, poses_last, K, inv_sigma2, nnratio, check_ori, th_low, min_matches, min_map, levelsup):
        """Both batched reference-keyframe calls.  store None: kfs[b] a keyframe dict (uploaded); else the KeyframeStore and kfs[b] a
        (slot, MapStore or None, mp_slots) tuple; None: the frame does not run."""
        count = len(kfs)
        assert len(poses_last) == count
        kfp = (C.POINTER(RefKeyframe if store is None else KfResident) * count)(); prs = (TrackRefKfParams * count)(); outs = (TrackRefKfOut * count)()
        res = (TrackRefKfResult * count)(); status = np.zeros(count, np.int32)
        keep = []
        for b in range(count):
            if kfs[b] is None:
                keep.append(None)
                continue
            if store is None:
                rk, ka = _ref_keyframe(kfs[b])
            else:
                rk, ka = KfResident(), []
                _kf_resident(kfs[b], rk, ka)
            pr, s2 = _refkf_params(poses_last[b], K, inv_sigma2, nnratio, check_ori, th_low, min_matches, min_map, levelsup)
            o, arrs = _refkf_out(self.ext.cap)
            kfp[b] = C.pointer(rk); prs[b] = pr; outs[b] = o
            keep.append((rk, ka, s2, arrs))
        if store is None:
            check(self.L.dvm_track_reference_keyframe_batch(self.t, self.ext.h, voc.h, count, kfp, prs, outs, res, _p(status)))
        else:
            check(self.L.dvm_track_reference_keyframe_batch_resident(self.t, self.ext.h, voc.h, store.h, count, kfp, prs, outs, res, _p(status)))
        out = []
        for b in range(count):
            d = self._refkf_result(res[b], None if keep[b] is None else keep[b][3])
            d["status"] = int(status[b])
            out.append(d)
        return out

    # ---- the first half
    def _track_arrays(self, B):
        """The extraction's and the search's output arrays for B frames at the extractor's capacity"""
        cap = self.ext.cap
        return dict(kps=np.empty((B, cap), KP_DTYPE), kps_un=np.empty((B, cap), KP_DTYPE), desc=np.empty((B, cap, 32), np.uint8), mp=np.empty((B, cap), np.int32),
                    dropped=np.empty((B, cap), np.int32))

    def _track_outs(self, B):
        """_track_arrays(B), the dvmh_track_out array pointing into them and the results: (arrays, outs, res)."""
        a, cap = self._track_arrays(B), self.ext.cap
        outs = (TrackOut * B)()
        for b in range(B):
            o = outs[b]
            o.kps, o.desc, o.cap, o.kps_un = a["kps"][b].ctypes.data, a["desc"][b].ctypes.data, cap, a["kps_un"][b].ctypes.data
            o.mp_c, o.dropped = a["mp"][b].ctypes.data, a["dropped"][b].ctypes.data
        return a, outs, (TrackResult * B)()

    @staticmethod
    def _track_ins(Tcw_preds, lasts, last_item):
        """dvmh_track_in[_resident] of the agents' (kps_l, mp_l, outlier_l or None, x): last_item(x) -> (what to keep alive, the address that
        goes where mps is).  Returns the array and what it points into."""
        ins = (TrackIn * len(lasts))()
        keep = []
        for b, (T, (kl, ml, ol, x)) in enumerate(zip(Tcw_preds, lasts)):
            T = np.ascontiguousarray(T, np.float32); kl = np.ascontiguousarray(kl, KP_DTYPE); ml = np.ascontiguousarray(ml, np.int32)
            ol = None if ol is None else np.ascontiguousarray(ol, np.uint8)
            x, addr = last_item(x)
            keep.append((T, kl, ml, ol, x))
            i = ins[b]
            i.Tcw_pred, i.Nl, i.kps_l, i.mp_l, i.outlier_l, i.mps = T.ctypes.data, len(kl), kl.ctypes.data, ml.ctypes.data, None if ol is None else ol.ctypes.data, addr
        return ins, keep

    @staticmethod
    def _track_result(r, a, b):
        """dvmh_track_result r and frame b of _track_outs' arrays as track() returns them"""
        n = r.n
        d = {k: getattr(r, k) for k in _TRACK_COUNTERS}
        d.update(kps=a["kps"][b, :n], kps_un=a["kps_un"][b, :n], desc=a["desc"][b, :n], mp=a["mp"][b, :n], dropped=a["dropped"][b, :n],
                 pose=np.array(r.pose[:], np.float64), Tcw=np.array(r.Tcw[:], np.float32))
        return d

    def _track_batch(self, io, imgs, ins, K, bounds, scale_factors, inv_sigma2, th, check_ori, lap, model=None, resident=False):
        """dvmh_track_with_motion_model_batch[_cam | _resident] on io = _track_outs(>= count); returns one dict per frame"""
        imgs = np.ascontiguousarray(imgs, np.uint8)
        count = imgs.shape[0]
        f4 = _f32(K, bounds, scale_factors, inv_sigma2)
        fn = self.H.dvmh_track_with_motion_model_batch_resident if resident else \
            self.H.dvmh_track_with_motion_model_batch if model is None else self.H.dvmh_track_with_motion_model_batch_cam
        a, outs, res = io
        check(fn(self.t, self.ext.h, self.device, count, imgs, imgs.shape[1], imgs.shape[2], imgs.strides[1], imgs.strides[0], int(lap[0]), int(lap[1]), f4[0],
                 *(() if model is None else (model,)), f4[1], f4[2], f4[3], len(f4[2]), float(th), int(check_ori), ins[0] if isinstance(ins, tuple) else ins, outs, res))
        return [self._track_result(res[b], a, b) for b in range(count)]

    # ---- the second half
    def _local_map_batch(self, tables, stores, frame_mps, th, far_points, th_far, want_track_points):
        """dvm_track_local_map_batch, or with stores dvm_track_local_map_batch_resident (tables: slot lists)"""
        count = len(tables)
        resident = stores is not None
        ths, fars, thfs = _per_frame(th, count), _per_frame(far_points, count), _per_frame(th_far, count)
        assert len(frame_mps) == count and len(ths) == count and len(fars) == count and len(thfs) == count and (not resident or len(stores) == count)
        ins = ((LocalMapInResident if resident else LocalMapIn) * count)(); outs = (LocalMapOut * count)(); res = (TrackLocalResult * count)()
        status = np.zeros(count, np.int32)
        keep = []
        for b in range(count):
            tab = np.ascontiguousarray(tables[b], np.int32 if resident else LOCAL_POINT_DTYPE)
            k = self._local_map_arrays(tab, frame_mps[b], want_track_points)
            keep.append(k)
            i = ins[b]
            if resident:
                i.store, i.slots = None if stores[b] is None else stores[b].h, tab.ctypes.data if len(tab) else None
            else:
                i.pts = tab.ctypes.data if len(tab) else None
            i.n, i.frame_mp, i.th, i.far_points, i.th_far = len(tab), k[1].ctypes.data, float(ths[b]), int(bool(fars[b])), float(thfs[b])
            outs[b].mp_out, outs[b].outlier, outs[b].track_pts = k[2].ctypes.data, k[3].ctypes.data, None if k[4] is None else k[4].ctypes.data
        fn = self.L.dvm_track_local_map_batch_resident if resident else self.L.dvm_track_local_map_batch
        check(fn(self.t, self.ext.h, count, ins, outs, res, _p(status)))
        return [self._local_result(res[b], keep[b], int(status[b])) for b in range(count)]

    @staticmethod
    def _local_map_arrays(tab, frame_mp, want_track_points):
        """one frame's table, frame_mp and the arrays the call writes: (table, frame_mp, mp, outlier, track_pts or None)"""
        fm = np.ascontiguousarray(frame_mp, np.int32)
        return (tab, fm, np.full(max(len(fm), 1), -1, np.int32), np.zeros(max(len(fm), 1), np.uint8),
                np.zeros(max(len(tab), 1), TRACK_DTYPE) if want_track_points else None)

    @staticmethod
    def _local_result(r, keep, status=None):
        """dvm_track_local_result r and _local_map_arrays' outputs as track_local_map returns them; status: the batched calls' (a frame with
        another status than DVM_TRACK_COMPLETE was skipped: zero counters, no arrays), None for the single call"""
        d = {k: getattr(r, k) for k in _LOCAL_COUNTERS}
        if status is not None:
            d["status"] = status
        if not status:
            tab, fm, mp, outl, tp = keep
            d.update(mp=mp[:len(fm)], outlier=outl[:len(fm)], pose=np.array(r.pose[:], np.float64), Tcw=np.array(r.Tcw[:], np.float32))
            if tp is not None:
                d["track_pts"] = tp[:len(tab)]
        return d

    @staticmethod
    def _refkf_result(res, arrs):
        """dvm_track_refkf_result and the outputs _refkf_out's arrays hold, as track_reference_keyframe returns them; arrs None: a frame that
        did not run (the counters, zero, without its status)"""
        if arrs is None:
            return {k: getattr(res, k) for k in _REFKF_COUNTERS if k != "status"}
        N, fo = res.n, arrs["fv_off"]
        out = {k: getattr(res, k) for k in _REFKF_COUNTERS}
        out.update(mp=arrs["mp"][:N], dropped=arrs["dropped"][:N], outlier=arrs["outlier"][:N], bow_ids=arrs["bow_ids"][:res.n_bow],
                   bow_vals=arrs["bow_vals"][:res.n_bow], fv_nodes=arrs["fv_nodes"][:res.n_fv], fv_off=fo[:res.n_fv + 1], fv_feat=arrs["fv_feat"][:fo[res.n_fv]],
                   pose=np.array(res.pose[:], np.float64), Tcw=np.array(res.Tcw[:], np.float32))
        return out


class Tracker(_TrackerBase):
    """dvm_tracker + dvmh_track_with_motion_model: Frame::Frame -> ExtractORB and Tracking::TrackWithMotionModel of one frame as ONE
    device chain behind one synchronisation (reference src/Frame.cc:371-411, src/Tracking.cc:2584-2667).  track and track_local_map call
    the single-frame C entry points; the resident forms are the batch of one."""

    def __init__(self, ext: "OrbExtractor", device=0, max_queries=None):
        self._open(ext, device, 1, lib().dvm_tracker_create, ext.cap, max_queries or ext.cap)

    def track(self, img, Tcw_pred, K, bounds, scale_factors, inv_sigma2, kps_l, mp_l, outlier_l, mps, th=15.0, check_ori=True, dist=None,
              lap=(0, 1000), model=None):
        """Tcw_pred: 7 floats (qx, qy, qz, qw, t).  model: a CameraModel (dvmh_track_with_motion_model_cam: the tracker is set to it and K,
        which may then be None, is not read), or None for the pinhole K.  Returns a dict: n, kps, desc, kps_un, mp (mvpMapPoints after the
        outlier drop), dropped, pose (7 doubles: t, q), and the counters of dvmh_track_result."""
        K = _need_K(K, model)
        img = np.ascontiguousarray(img, np.uint8)
        a, res = self._track_arrays(1), TrackResult()       # (fresh per call: a result stays valid after the next call)
        kps_l = np.ascontiguousarray(kps_l, KP_DTYPE); mp_l = np.ascontiguousarray(mp_l, np.int32)
        outl = None if outlier_l is None else np.ascontiguousarray(outlier_l, np.uint8)
        f4 = _f32(Tcw_pred, K, bounds, scale_factors, inv_sigma2)
        mps = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
        fn = self.H.dvmh_track_with_motion_model if model is None else self.H.dvmh_track_with_motion_model_cam
        check(fn(self.t, self.ext.h, self.device, img, img.shape[0], img.shape[1], img.strides[0], int(lap[0]), int(lap[1]), f4[0], f4[1],
                 *(() if model is None else (model,)), f4[2], dist, f4[3], f4[4], len(f4[3]), len(kps_l), kps_l, mp_l, outl, mps, float(th), int(check_ori),
                 a["kps"][0], a["desc"][0], self.ext.cap, a["kps_un"][0], a["mp"][0], a["dropped"][0], res))
        return self._track_result(res, a, 0)

    def track_resident(self, img, Tcw_pred, K, bounds, scale_factors, inv_sigma2, kps_l, mp_l, outlier_l, store, th=15.0, check_ori=True, lap=(0, 1000)):
        """dvmh_track_with_motion_model_batch_resident for one frame: Tracker.track with LastFrame's map points given as slots of `store` (a
        MapStore) in mp_l.  Under a camera model set with set_camera_model K may be None.  Returns what track() returns, mp / dropped as slots."""
        ins, keep = TrackerBatch.prepare_resident([Tcw_pred], [(kps_l, mp_l, outlier_l, store)])
        img = np.ascontiguousarray(img, np.uint8)
        return self._track_batch(self._track_outs(1), img[None], ins, K, bounds, scale_factors, inv_sigma2, th, check_ori, lap, resident=True)[0]

    def track_local_map(self, pts, frame_mp, th=1.0, far_points=False, th_far=0.0, want_track_points=False):
        """dvm_track_local_map: Tracking::TrackLocalMap of the frame the last track() call tracked (reference src/Tracking.cc:2668-2740) as
        ONE device chain.  pts: LOCAL_POINT_DTYPE array (the local map); frame_mp [n]: per keypoint the index into pts of the point the
        frame holds, or -1.  Returns a dict: mp (mvpMapPoints after the search), outlier (mvbOutlier), track_pts (TRACK_DTYPE per entry,
        if asked), the counters of dvm_track_local_result, pose (7 doubles: t, q) and Tcw (7 floats: q, t)."""
        keep = self._local_map_arrays(np.ascontiguousarray(pts, LOCAL_POINT_DTYPE), frame_mp, want_track_points)
        pts, fm, mp, outl, tp = keep
        res = TrackLocalResult()
        check(self.L.dvm_track_local_map(self.t, self.ext.h, pts if len(pts) else None, len(pts), fm, float(th), int(bool(far_points)), float(th_far), mp, outl, tp, res))
        return self._local_result(res, keep)

    def track_local_map_resident(self, store, slots, frame_mp, th=1.0, far_points=False, th_far=0.0, want_track_points=False):
        """dvm_track_local_map_batch_resident for the one frame of the last track() / track_resident(): Tracker.track_local_map with the local map
        given as slots of `store`.  Returns what track_local_map returns plus status."""
        return self._local_map_batch([slots], [store], [frame_mp], th, far_points, th_far, want_track_points)[0]

    def reserve_reference_keyframe(self, n):
        """dvm_tracker_reserve_reference_keyframe: the reference-keyframe chain's working set for keyframes of up to n keypoints."""
        check(self.L.dvm_tracker_reserve_reference_keyframe(self.t, int(n)))

    def track_reference_keyframe(self, voc, kf, pose_last, img=None, K=None, bounds=None, inv_sigma2=None, dist=None, nnratio=0.7, check_ori=True,
                                 th_low=50, min_matches=15, min_map=10, levelsup=4, lap=(0, 1000), model=None):
        """dvm_track_reference_keyframe: Tracking::TrackReferenceKeyFrame (reference src/Tracking.cc:2461-2520) as ONE device chain.
        voc: a Vocabulary; kf: dict(kps (mvKeysUn), desc, mp (map-point ids or -1), pos [n, 3], n_obs, bad (optional), fv (mFeatVec as
        vocab_transform_host returns it)); pose_last: mLastFrame.GetPose() as 7 floats (qx, qy, qz, qw, t).  With img: dvm_track_begin on it,
        then the chain (form a: the no-motion-model case); without: the chain on the frame of the last track() (form b: the motion model
        failed).  K: fx fy cx cy; bounds, dist: form (a).  model: a CameraModel -- with img the tracker is set to it before the begin (form (b)
        runs on the model of the frame's track() call); K may then be None (it is not read under KannalaBrandt8).  Returns a dict: the counters of dvm_track_refkf_result, mp (mvpMapPoints after the
        outlier drop), dropped, outlier, bow_ids / bow_vals / fv_nodes / fv_off / fv_feat (ComputeBoW), pose (7 doubles: t, q), Tcw (7 floats:
        q, t) and, in form (a), kps / desc / kps_un."""
        cap = self.ext.cap
        if model is not None:
            K = model.p[:4] if K is None else K
            if img is not None:
                self.set_camera_model(model)
        if img is not None:
            img = np.ascontiguousarray(img, np.uint8)
            check(self.L.dvm_track_begin(self.t, self.ext.h, img.ctypes.data, img.shape[0], img.shape[1], img.strides[0], int(lap[0]), int(lap[1])))
        rk, keep = _ref_keyframe(kf)
        pr, s2 = _refkf_params(pose_last, K, inv_sigma2, nnratio, check_ori, th_low, min_matches, min_map, levelsup)
        if bounds is not None:
            pr.bounds[:] = [float(v) for v in np.asarray(bounds, np.float32)]
        pr.dist = None if dist is None else C.cast(C.pointer(dist), C.c_void_p)
        kps = np.empty(cap, KP_DTYPE); kun = np.empty(cap, KP_DTYPE); desc = np.empty((cap, 32), np.uint8)
        o, arrs = _refkf_out(cap)
        o.kps, o.desc, o.cap, o.kps_un = kps.ctypes.data, desc.ctypes.data, cap, kun.ctypes.data
        res = TrackRefKfResult()
        check(self.L.dvm_track_reference_keyframe(self.t, self.ext.h, voc.h, rk, pr, o, res))
        N = res.n
        out = self._refkf_result(res, arrs)
        if img is not None:
            out.update(kps=kps[:N], desc=desc[:N], kps_un=kun[:N])
        return out


    def reserve_reference_keyframe_batch(self, total):
        """dvm_tracker_reserve_reference_keyframe_batch on the single-frame tracker: the working set track_reference_keyframe_resident runs on."""
        check(self.L.dvm_tracker_reserve_reference_keyframe_batch(self.t, int(total)))

    def track_reference_keyframe_resident(self, voc, store, kf, pose_last, K, inv_sigma2, nnratio=0.7, check_ori=True, th_low=50, min_matches=15,
                                          min_map=10, levelsup=4, model=None):
        """dvm_track_reference_keyframe_batch_resident for the one frame of the last track() (form (b) of track_reference_keyframe: the motion
        model failed): the reference keyframe as (slot, MapStore or None, mp_slots) of `store` (a KeyframeStore).  Needs
        reserve_reference_keyframe_batch.  Returns what track_reference_keyframe returns in form (b), mp / dropped as map-store slots."""
        K = _need_K(K, model)
        return self._refkf_batch(voc, [kf], store, [pose_last], K, inv_sigma2, nnratio, check_ori, th_low, min_matches, min_map, levelsup)[0]


class TrackerBatch(_TrackerBase):
    """dvm_tracker_create_batch + dvmh_track_with_motion_model_batch: the tracked frames of up to max_frames agents as ONE chain of batched
    launches.  ext: an OrbExtractor with max_batch >= max_frames."""

    def __init__(self, ext: "OrbExtractor", max_frames, device=0):
        self._open(ext, device, max_frames, lib().dvm_tracker_create_batch, int(max_frames), ext.cap, ext.cap)
        self._io = self._track_outs(self.max_frames)       # the first half's outputs: track() returns views into them
        a, self.outs, self.res = self._io
        self.kps, self.kun, self.desc, self.mp, self.dropped = a["kps"], a["kps_un"], a["desc"], a["mp"], a["dropped"]

    def prepare(self, Tcw_preds, lasts):
        """lasts: per agent (kps_l, mp_l, outlier_l or None, mps).  Returns the marshalled dvmh_track_in array (keep it alive with its arrays)."""
        def mps_of(mps):
            mps = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
            return mps, mps.ctypes.data
        return self._track_ins(Tcw_preds, lasts, mps_of)

    @staticmethod
    def prepare_resident(Tcw_preds, lasts):
        """lasts: per agent (kps_l, mp_l as store slots, outlier_l or None, MapStore).  Returns the marshalled dvmh_track_in_resident array."""
        return _TrackerBase._track_ins(Tcw_preds, lasts, lambda store: (store, store.h))

    def track(self, imgs, ins, K, bounds, scale_factors, inv_sigma2, th=15.0, check_ori=True, lap=(0, 1000), model=None):
        """imgs [count, rows, cols] u8; ins: prepare()'s array; model: as Tracker.track takes it, one for all frames
        (dvmh_track_with_motion_model_batch_cam).  Returns one dict per frame (views into this object's arrays)."""
        return self._track_batch(self._io, imgs, ins, _need_K(K, model), bounds, scale_factors, inv_sigma2, th, check_ori, lap, model=model)

    def track_resident(self, imgs, ins, K, bounds, scale_factors, inv_sigma2, th=15.0, check_ori=True, lap=(0, 1000)):
        """dvmh_track_with_motion_model_batch_resident: TrackerBatch.track with every agent's map points in a MapStore.  ins: prepare_resident()'s
        array.  Returns one dict per frame as track() does, mp / dropped as store slots."""
        return self._track_batch(self._io, imgs, ins, K, bounds, scale_factors, inv_sigma2, th, check_ori, lap, resident=True)

    def track_local_map(self, tables, frame_mps, th=1.0, far_points=False, th_far=0.0, want_track_points=False):
        """dvm_track_local_map_batch: Tracking::TrackLocalMap of every frame the last track() call tracked, as ONE device chain.  tables [count]:
        LOCAL_POINT_DTYPE arrays; frame_mps [count]: per keypoint the index into that frame's table, or -1; th / far_points / th_far: one value
        for all frames or one per frame.  Returns one dict per frame: status (DVM_TRACK_COMPLETE = 0, else the first half's status and the
        frame was skipped: zero counters, no arrays) and, for completed frames, what Tracker.track_local_map returns."""
        return self._local_map_batch(tables, None, frame_mps, th, far_points, th_far, want_track_points)

    def track_local_map_resident(self, stores, slot_lists, frame_mps, th=1.0, far_points=False, th_far=0.0, want_track_points=False):
        """dvm_track_local_map_batch_resident: TrackerBatch.track_local_map with every frame's table given as slots of its MapStore."""
        return self._local_map_batch(slot_lists, stores, frame_mps, th, far_points, th_far, want_track_points)

    def reserve_reference_keyframe(self, total):
        """dvm_tracker_reserve_reference_keyframe_batch: the batched reference-keyframe chain's working set for `total` keyframe keypoints
        per call (the sum over its keyframes of each one's size rounded up to 64), per-frame arrays for max_frames frames."""
        check(self.L.dvm_tracker_reserve_reference_keyframe_batch(self.t, int(total)))

    def track_reference_keyframe(self, voc, kfs, poses_last, K, inv_sigma2, nnratio=0.7, check_ori=True, th_low=50, min_matches=15, min_map=10,
                                 levelsup=4):
        """dvm_track_reference_keyframe_batch: Tracking::TrackReferenceKeyFrame of the frames of the last track() call that need it, as ONE
        device chain.  kfs [count]: a keyframe dict as Tracker.track_reference_keyframe takes it, or None for a frame that does not run;
        poses_last [count]: mLastFrame.GetPose() as 7 floats (qx, qy, qz, qw, t), read where kfs[b] is not None.  Returns one dict per frame:
        status (the chain's for a frame that ran, else the first half's: zero counters, no arrays) and, for a frame that ran, what
        Tracker.track_reference_keyframe returns in form (b)."""
        return self._refkf_batch(voc, kfs, None, poses_last, K, inv_sigma2, nnratio, check_ori, th_low, min_matches, min_map, levelsup)

    def track_reference_keyframe_resident(self, voc, store, kfs, poses_last, K, inv_sigma2, nnratio=0.7, check_ori=True, th_low=50, min_matches=15,
                                          min_map=10, levelsup=4):
        """dvm_track_reference_keyframe_batch_resident: track_reference_keyframe with every reference keyframe given as a slot of `store` (a
        KeyframeStore): kfs [count]: (slot, MapStore or None, mp_slots), or None for a frame that does not run.  Returns what
        track_reference_keyframe returns, mp / dropped as map-store slots."""
        return self._refkf_batch(voc, kfs, store, poses_last, K, inv_sigma2, nnratio, check_ori, th_low, min_matches, min_map, levelsup)


MP_OBS_DTYPE = np.dtype([("kf", "<i4"), ("kp", "<i4")])                                   # == dvm_mp_obs
MP_REFRESH_KF_DTYPE = np.dtype([("slot", "<i4"), ("flags", "<u4"), ("ow", "<f4", (3,))])    # == dvm_mp_refresh_kf
MPR_KF_BAD, MPR_DESCRIPTOR, MPR_GEOMETRY = 1, 1, 2


class MpRefresh(C.Structure):
    """dvm_mp_refresh (include/dvmslam_hip.h)"""
    _fields_ = [("n_points", C.c_int32), ("n_kfs", C.c_int32), ("n_obs", C.c_int32), ("what", C.c_uint32), ("mp_slot", C.c_void_p),
                ("obs_off", C.c_void_p), ("obs", C.c_void_p), ("ref_obs", C.c_void_p), ("kfs", C.c_void_p), ("is_new", C.c_void_p),
                ("new_pos", C.c_void_p), ("best_obs_out", C.c_void_p), ("best_median_out", C.c_void_p), ("geometry_out", C.c_void_p)]


# ---- an agent's map points resident on the device (dvm_map_store, include/dvmslam_hip.h), read by the two tracked-frame halves above
class MapStore:
    """dvm_map_store: `capacity` slots of LOCAL_POINT_DTYPE records in device memory.  update() writes records to slots (asynchronous; every
    later call that reads the store sees it), read() returns slots.  Calls on one store are not concurrent."""

    def __init__(self, capacity, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        f = self.L.dvm_map_store_create
        f.restype = C.c_int32; f.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
        check(f(int(device), int(capacity), C.byref(self.h)))

    @property
    def capacity(self):
        f = self.L.dvm_map_store_capacity
        f.restype = C.c_int32; f.argtypes = [C.c_void_p]
        return f(self.h)

    def update(self, slots, records):
        slots = np.ascontiguousarray(slots, np.int32); records = np.ascontiguousarray(records, LOCAL_POINT_DTYPE)
        assert slots.ndim == 1 and slots.shape == records.shape
        f = self.L.dvm_map_store_update
        f.restype = C.c_int32; f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        check(f(self.h, len(slots), _p(slots), _p(records)))

    def read(self, slots):
        slots = np.ascontiguousarray(slots, np.int32)
        out = np.zeros(len(slots), LOCAL_POINT_DTYPE)
        f = self.L.dvm_map_store_read
        f.restype = C.c_int32; f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        check(f(self.h, len(slots), _p(slots), _p(out)))
        return out

    def refresh(self, kf_store, mp_slots, obs_off, obs, ref_obs, kfs, is_new=None, new_pos=None, what=3, want_geometry=False, out=None):
        """dvm_map_store_refresh: ComputeDistinctiveDescriptors + UpdateNormalAndDepth into the records of mp_slots, from the descriptor
        rows kf_store's slots hold.  obs (MP_OBS_DTYPE) in CSR order by obs_off [n + 1]; ref_obs [n]: mpRefKF's observation inside each
        point's list; kfs (MP_REFRESH_KF_DTYPE); is_new [n] + new_pos [n, 3]: points that enter the store with this call.  Returns
        dict(best_obs [n] (-1: descriptor not written), best_median [n], geometry [n, 8] or None) -- `out` itself when the caller
        brings the arrays (int32 [n], int32 [n], float32 [n, 8] or None)."""
        mp_slots = np.ascontiguousarray(mp_slots, np.int32); obs_off = np.ascontiguousarray(obs_off, np.int32)
        obs = np.ascontiguousarray(obs, MP_OBS_DTYPE); ref_obs = np.ascontiguousarray(ref_obs, np.int32)
        kfs = np.ascontiguousarray(kfs, MP_REFRESH_KF_DTYPE)
        n = len(mp_slots)
        assert obs_off.shape == (n + 1,) and ref_obs.shape == (n,)
        if is_new is not None:
            is_new = np.ascontiguousarray(is_new, np.uint8); new_pos = np.ascontiguousarray(new_pos, np.float32).reshape(-1, 3)
            assert is_new.shape == (n,) and new_pos.shape == (n, 3)
        if out is None:
            out = dict(best_obs=np.zeros(n, np.int32), best_median=np.zeros(n, np.int32), geometry=np.zeros((n, 8), np.float32) if want_geometry else None)
        want_geometry = out["geometry"] is not None
        assert out["best_obs"].shape == out["best_median"].shape == (n,) and out["best_obs"].dtype == out["best_median"].dtype == np.int32
        assert not want_geometry or (out["geometry"].shape == (n, 8) and out["geometry"].dtype == np.float32 and out["geometry"].flags.c_contiguous)
        a = MpRefresh(n, len(kfs), len(obs), int(what), mp_slots.ctypes.data, obs_off.ctypes.data, obs.ctypes.data, ref_obs.ctypes.data, kfs.ctypes.data,
                      None if is_new is None else is_new.ctypes.data, None if is_new is None else new_pos.ctypes.data, out["best_obs"].ctypes.data,
                      out["best_median"].ctypes.data, out["geometry"].ctypes.data if want_geometry else None)
        f = self.L.dvm_map_store_refresh
        f.restype = C.c_int32; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        check(f(self.h, kf_store.h, C.byref(a)))
        return out

    def last_refresh_bytes(self):
        """(host to device, device to host) of the last refresh."""
        up, down = C.c_int64(0), C.c_int64(0)
        f = self.L.dvm_map_store_last_refresh_bytes
        f.restype = C.c_int32; f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        check(f(self.h, C.byref(up), C.byref(down)))
        return up.value, down.value

    def profile(self, enable=True):
        """HIP-event timing of the refresh kernel on / off (measurement only)."""
        f = self.L.dvm_map_store_profile
        f.restype = C.c_int32; f.argtypes = [C.c_void_p, C.c_int32]
        check(f(self.h, int(bool(enable))))

    def last_refresh_ms(self):
        ms = C.c_float(0)
        f = self.L.dvm_map_store_last_refresh_ms
        f.restype = C.c_int32; f.argtypes = [C.c_void_p, C.c_void_p]
        check(f(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            f = self.L.dvm_map_store_destroy
            f.restype = None; f.argtypes = [C.c_void_p]
            f(self.h)
            self.h = C.c_void_p()

    __del__ = close


BA_OBS_DTYPE = np.dtype([("pose", "<i4"), ("point", "<i4"), ("kp", "<i4")])      # == dvm_ba_obs


class BaWindowResident(C.Structure):
    """dvm_ba_window_resident (include/dvmslam_hip.h)"""
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32), ("iterations", C.c_int32),
                ("poses", C.c_void_p), ("fixed", C.c_void_p), ("keyframes", C.c_void_p), ("kf_slot", C.c_void_p), ("ow", C.c_void_p),
                ("points", C.c_void_p), ("mp_slot", C.c_void_p), ("obs", C.c_void_p), ("ref_edge", C.c_void_p), ("cam", BaCamera),
                ("chi2_erase", C.c_double), ("poses_out", C.c_void_p), ("points_out", C.c_void_p), ("edge_chi2_out", C.c_void_p),
                ("depth_positive_out", C.c_void_p), ("geometry_out", C.c_void_p), ("point_dirty_out", C.c_void_p), ("ow_out", C.c_void_p)]


class BaResidentBatch:
    """K resident windows marshalled once into the dvm_ba_window_resident array (BaWindowBatch's counterpart).  problems: the dicts of
    ba_optimize_windows without points / edges, with kf_slots [P] + keyframe_store (a KeyframeStore), mp_slots [L] + map_store (a MapStore),
    obs (BA_OBS_DTYPE), ref_edge [L] or None, ow [P, 3] or None, chi2_erase (default 5.991), model (a CameraModel) or intrinsics;
    want_geometry=False: geometry_out and ow_out are NULL (the commit needs neither on the host) and the result arrays stay zeros."""

    def __init__(self, problems):
        K = len(problems)
        self.K = K
        self.wins = (BaWindowResident * max(K, 1))()
        self.stats = (BaStats * max(K, 1))()
        self.models = None
        if any(pr.get("model") is not None for pr in problems):
            self.models = (CameraModel * max(K, 1))()
            for k, pr in enumerate(problems):
                m = pr.get("model")
                self.models[k] = m if m is not None else CameraModel.pinhole(*[float(v) for v in pr["intrinsics"]])
        self.keep, self.outs = [], []
        for k, pr in enumerate(problems):
            poses = np.ascontiguousarray(pr["poses"], np.float64).reshape(-1, 7); fixed = np.ascontiguousarray(pr["fixed"], np.uint8)
            kf_slots = np.ascontiguousarray(pr["kf_slots"], np.int32); mp_slots = np.ascontiguousarray(pr["mp_slots"], np.int32)
            obs = np.ascontiguousarray(pr["obs"], BA_OBS_DTYPE)
            assert len(kf_slots) == len(poses) == len(fixed)
            P, L, E = len(poses), len(mp_slots), len(obs)
            ref = None if pr.get("ref_edge") is None else np.ascontiguousarray(pr["ref_edge"], np.int32)
            ow = None if pr.get("ow") is None else np.ascontiguousarray(pr["ow"], np.float32).reshape(-1, 3)
            assert ref is None or len(ref) == L
            assert ow is None or len(ow) == P
            o = dict(poses=np.zeros((P, 7), np.float64), points=np.zeros((L, 3), np.float64), edge_chi2=np.zeros(E, np.float64),
                     depth_positive=np.zeros(E, np.uint8), geometry=np.zeros((L, 8), np.float32), point_dirty=np.zeros(L, np.uint8),
                     ow=np.zeros((P, 3), np.float32))
            self.keep.append((poses, fixed, kf_slots, mp_slots, obs, ref, ow, pr.get("keyframe_store"), pr.get("map_store"))); self.outs.append(o)
            w = self.wins[k]
            w.n_poses, w.n_points, w.n_edges, w.iterations = P, L, E, int(pr["iterations"])
            w.poses, w.fixed, w.kf_slot, w.mp_slot, w.obs = poses.ctypes.data, fixed.ctypes.data, kf_slots.ctypes.data, mp_slots.ctypes.data, obs.ctypes.data
            w.keyframes = pr["keyframe_store"].h if pr.get("keyframe_store") is not None else None
            w.points = pr["map_store"].h if pr.get("map_store") is not None else None
            w.ref_edge = ref.ctypes.data if ref is not None else None
            w.ow = ow.ctypes.data if ow is not None else None
            intr = pr["intrinsics"] if pr.get("model") is None else list(pr["model"].p[:4])
            w.cam = BaCamera(*[float(v) for v in intr], float(pr["huber_delta"]))
            w.chi2_erase = float(pr.get("chi2_erase", 5.991))
            w.poses_out, w.points_out, w.edge_chi2_out, w.depth_positive_out = (o["poses"].ctypes.data, o["points"].ctypes.data, o["edge_chi2"].ctypes.data,
                                                                                o["depth_positive"].ctypes.data)
            w.point_dirty_out = o["point_dirty"].ctypes.data
            if pr.get("want_geometry", True):
                w.geometry_out, w.ow_out = o["geometry"].ctypes.data, o["ow"].ctypes.data

    results = BaWindowBatch.results


class BaResident:
    """dvm_ba_resident: LocalBundleAdjustment windows that read a KeyframeStore and a MapStore by slot and write their result back into the
    MapStore on the device.  optimize() is ba_optimize_windows(fast=True) on what the slots hold (the same bits) plus, per window,
    `geometry` [L, 8] (pos, normal, min_dist, max_dist of the clean, used points; zeros elsewhere), `point_dirty` [L] and `ow` [P, 3];
    commit(k) queues the write of window k's geometry (-1: every window not yet committed) into the map store's records."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        vp, i32 = C.c_void_p, C.c_int32
        for name, args in (("create", [i32, vp]), ("optimize", [vp, vp, vp, i32, vp, vp]), ("commit", [vp, i32]), ("last_bytes", [vp, vp, vp])):
            f = getattr(self.L, "dvm_ba_resident_" + name)
            f.restype = i32; f.argtypes = args
        self.L.dvm_ba_resident_destroy.restype = None; self.L.dvm_ba_resident_destroy.argtypes = [vp]
        check(self.L.dvm_ba_resident_create(int(device), C.byref(self.h)))

    def run(self, batch, stop_flag=None, collect=True):
        """The bare library call on a BaResidentBatch."""
        sf = _p(stop_flag) if stop_flag is not None else None
        check(self.L.dvm_ba_resident_optimize(self.h, C.addressof(batch.wins), None if batch.models is None else C.addressof(batch.models), batch.K, sf,
                                              C.addressof(batch.stats)))
        return batch.results() if collect else None

    def optimize(self, problems, stop_flag=None):
        return self.run(BaResidentBatch(problems), stop_flag)

    def commit(self, k=-1):
        check(self.L.dvm_ba_resident_commit(self.h, int(k)))

    def last_bytes(self):
        """(host to device, device to host) of the last optimize."""
        up, down = C.c_int64(0), C.c_int64(0)
        check(self.L.dvm_ba_resident_last_bytes(self.h, C.byref(up), C.byref(down)))
        return up.value, down.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.dvm_ba_resident_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close


TRACKED_POINT_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("depth", "<f4"), ("view_cos", "<f4"), ("level", "<i4"),
                                ("in_view", "u1"), ("bad", "u1"), ("pad", "u1", (2,)), ("desc", "u1", (32,)), ("n_obs", "<i4")])


def search_by_projection_points(kps, desc, mp, claimed_obs, bounds, scale_factors, pts, th, nnratio=0.8, far_points=False,
                                th_far=0.0, device=0):
    """dvm_host::ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) -- reference
    ORBmatcher.cc:44-205.  Returns (nmatches, updated mvpMapPoints, #host re-queries)."""
    H = host_lib()
    vp = C.c_void_p
    H.dvmh_search_by_projection_points.restype = C.c_int32
    H.dvmh_search_by_projection_points.argtypes = [C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_int32, vp, C.c_int32,
                                                   C.c_float, C.c_float, C.c_int32, C.c_float, vp]
    kps = np.ascontiguousarray(kps, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
    mpc = np.array(mp, np.int32, copy=True)
    co = np.ascontiguousarray(claimed_obs, np.uint8)
    b = np.ascontiguousarray(bounds, np.float32); sf = np.ascontiguousarray(scale_factors, np.float32)
    pts = np.ascontiguousarray(pts, TRACKED_POINT_DTYPE)
    req = C.c_int32(0)
    n = H.dvmh_search_by_projection_points(device, len(kps), _p(kps), _p(desc), _p(mpc), _p(co), _p(b), _p(sf), len(sf), _p(pts),
                                           len(pts), float(th), float(nnratio), int(far_points), float(th_far), C.byref(req))
    if n < 0:
        check(n)
    return n, mpc, req.value


def distinctive_descriptors(desc, off):
    """dvm_distinctive_descriptors: MapPoint::ComputeDistinctiveDescriptors for a batch of map points (CSR offsets).
    Returns (best_idx, best_median)."""
    L = lib()
    L.dvm_distinctive_descriptors.restype = C.c_int32
    L.dvm_distinctive_descriptors.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); off = np.ascontiguousarray(off, np.int32)
    n = len(off) - 1
    bi = np.zeros(max(n, 1), np.int32); bm = np.zeros(max(n, 1), np.int32)
    dummy = np.zeros((1, 32), np.uint8)
    check(L.dvm_distinctive_descriptors(_p(desc if len(desc) else dummy), _p(off), n, _p(bi), _p(bm), 0, None))
    return bi[:n], bm[:n]


class Vocabulary:
    """dvm_vocab_*: DBoW2 vocabulary tree resident on the device, per-feature transform."""

    def __init__(self, voc, device=0):
        L = lib()
        vp, i32 = C.c_void_p, C.c_int32
        L.dvm_vocab_create.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, C.POINTER(vp)]
        L.dvm_vocab_destroy.argtypes = [vp]; L.dvm_vocab_destroy.restype = None
        L.dvm_vocab_transform.argtypes = [vp, vp, i32, i32, vp, vp, vp, i32, vp]
        self.L, self.h = L, vp()
        self.keep = [np.ascontiguousarray(voc[k]) for k in ("child_off", "children", "desc", "weight", "word_id")]
        check(L.dvm_vocab_create(device, voc["n_nodes"], *[_p(a) for a in self.keep], voc["L"], C.byref(self.h)))

    def transform(self, features, levelsup, on_device=False):
        """(word id, node id, weight) per feature.  on_device: the form on device pointers (torch tensors, the null stream)."""
        f = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
        n = len(f)
        if on_device and n:
            import torch
            df = torch.from_numpy(f).cuda()
            dw = torch.full((n,), -7, dtype=torch.int32, device="cuda"); dn = torch.full_like(dw, -7)
            dwt = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            check(self.L.dvm_vocab_transform(self.h, df.data_ptr(), n, levelsup, dw.data_ptr(), dn.data_ptr(), dwt.data_ptr(), 1, None))
            torch.cuda.synchronize()
            return dw.cpu().numpy(), dn.cpu().numpy(), dwt.cpu().numpy()
        word = np.zeros(max(n, 1), np.int32); node = np.zeros(max(n, 1), np.int32); w = np.zeros(max(n, 1), np.float64)
        check(self.L.dvm_vocab_transform(self.h, _p(f) if n else None, n, levelsup, _p(word), _p(node), _p(w), 0, None))
        return word[:n], node[:n], w[:n]

    def close(self):
        if self.h:
            self.L.dvm_vocab_destroy(self.h)
            self.h = None


def vocab_transform_host(voc, features, levelsup, device=0):
    """dvm_host::ORBVocabulary::transform (host C++ mirror): returns dict(bow_ids, bow_vals, fv_nodes, fv_off, fv_feat)."""
    H = host_lib()
    vp, i32 = C.c_void_p, C.c_int32
    H.dvmh_vocab_transform.restype = i32
    H.dvmh_vocab_transform.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    f = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
    n = len(f)
    bi = np.zeros(n + 1, np.int32); bv = np.zeros(n + 1, np.float64); fn = np.zeros(n + 1, np.int32)
    fo = np.zeros(n + 2, np.int32); ff = np.zeros(n + 1, np.int32)
    nb = C.c_int32(0); nf = C.c_int32(0)
    check(H.dvmh_vocab_transform(device, voc["n_nodes"], _p(voc["child_off"]), _p(voc["children"]), _p(voc["desc"]),
                                 _p(voc["weight"]), _p(voc["word_id"]), voc["L"], _p(f), n, levelsup, _p(bi), _p(bv),
                                 C.byref(nb), _p(fn), _p(fo), _p(ff), C.byref(nf)))
    return dict(bow_ids=bi[:nb.value], bow_vals=bv[:nb.value], fv_nodes=fn[:nf.value], fv_off=fo[:nf.value + 1],
                fv_feat=ff[:fo[nf.value]])


class HostVocabulary:
    """dvm_host::ORBVocabulary loaded from DBoW2's text format (loadFromTextFile, TemplatedVocabulary.h:1211-1286) and kept on the device."""

    def __init__(self, filename, device=0):
        H = host_lib()
        H.dvmh_vocab_load_text.restype = C.c_void_p
        H.dvmh_vocab_load_text.argtypes = [C.c_int32, C.c_char_p, C.c_void_p]
        info = np.zeros(4, np.int32)
        self.h = C.c_void_p(H.dvmh_vocab_load_text(device, os.fsencode(filename), _p(info)))
        if not self.h.value:
            raise DvmError(-1, f"{filename}: not a DBoW2 text vocabulary (or the device refused it)")
        self.k, self.L, self.nodes, self.words = (int(x) for x in info)

    def transform(self, features, levelsup):
        H = host_lib()
        H.dvmh_vocab_transform_loaded.restype = C.c_int32; H.dvmh_vocab_transform_loaded.argtypes = None
        f = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
        n = len(f)
        bi = np.zeros(n + 1, np.int32); bv = np.zeros(n + 1, np.float64); fn = np.zeros(n + 1, np.int32)
        fo = np.zeros(n + 2, np.int32); ff = np.zeros(n + 1, np.int32)
        nb = C.c_int32(0); nf = C.c_int32(0)
        check(H.dvmh_vocab_transform_loaded(self.h, _p(f), C.c_int32(n), C.c_int32(levelsup), _p(bi), _p(bv), C.byref(nb), _p(fn), _p(fo), _p(ff), C.byref(nf)))
        return dict(bow_ids=bi[:nb.value], bow_vals=bv[:nb.value], fv_nodes=fn[:nf.value], fv_off=fo[:nf.value + 1], fv_feat=ff[:fo[nf.value]])

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            f = host_lib().dvmh_vocab_destroy; f.restype = None; f.argtypes = [C.c_void_p]
            f(self.h); self.h = C.c_void_p()

    __del__ = close


def bow_score_host(ids1, vals1, ids2, vals2):
    H = host_lib()
    H.dvmh_bow_score.restype = C.c_double
    H.dvmh_bow_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    a = np.ascontiguousarray(ids1, np.int32); b = np.ascontiguousarray(vals1, np.float64)
    c = np.ascontiguousarray(ids2, np.int32); d = np.ascontiguousarray(vals2, np.float64)
    return H.dvmh_bow_score(_p(a), _p(b), len(a), _p(c), _p(d), len(c))


def sim3_hypotheses(P1c, P2c, max_err1, max_err2, K1, K2, triples, fix_scale=False, device=0):
    """dvm_sim3_hypotheses: Sim3Solver::ComputeSim3 + CheckInliers for H minimal sets in one launch.
    Returns (T12[H,13] = s, R row-major, t; n_inliers[H]; mask[H,N])."""
    L = lib()
    vp, i32 = C.c_void_p, C.c_int32
    L.dvm_sim3_hypotheses.restype = i32
    L.dvm_sim3_hypotheses.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp]
    a = [np.ascontiguousarray(x, np.float32) for x in (P1c, P2c, max_err1, max_err2, K1, K2)]
    tr = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    N, H = len(a[0]), len(tr)
    T = np.zeros((H, 13), np.float32); nin = np.zeros(H, np.int32); mask = np.zeros((H, N), np.uint8)
    check(L.dvm_sim3_hypotheses(device, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), N, _p(a[4]), _p(a[5]), _p(tr), H, int(fix_scale),
                                _p(T), _p(nin), _p(mask)))
    return T, nin, mask


def sim3_hypotheses_cam(P1c, P2c, max_err1, max_err2, model1, model2, triples, fix_scale=False, device=0):
    """dvm_sim3_hypotheses_cam: sim3_hypotheses with a CameraModel per keyframe (any pair of pinhole / KannalaBrandt8); T12 does not
    depend on the models.  Returns (T12[H,13]; n_inliers[H]; mask[H,N])."""
    L = lib()
    vp, i32 = C.c_void_p, C.c_int32
    L.dvm_sim3_hypotheses_cam.restype = i32
    L.dvm_sim3_hypotheses_cam.argtypes = [i32, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp]
    a = [np.ascontiguousarray(x, np.float32) for x in (P1c, P2c, max_err1, max_err2)]
    tr = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
    N, H = len(a[0]), len(tr)
    T = np.zeros((H, 13), np.float32); nin = np.zeros(H, np.int32); mask = np.zeros((H, N), np.uint8)
    check(L.dvm_sim3_hypotheses_cam(device, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), N, C.addressof(model1), C.addressof(model2), _p(tr), H,
                                    int(fix_scale), _p(T), _p(nin), _p(mask)))
    return T, nin, mask


PG_EDGE_DTYPE = np.dtype([("vi", "<i4"), ("vj", "<i4"), ("Sji", "<f8", (8,))])


class PgStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("total_trials", C.c_int32), ("stop_reason", C.c_int32), ("levels", C.c_int32),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double), ("tile_fill", C.c_double),
                ("ms_structure", C.c_double), ("ms_optimize", C.c_double), ("chi2_per_iter", C.c_double * 32),
                ("trials_per_iter", C.c_int32 * 32)]


def pose_graph_optimize(S, fixed, edges_v, edges_meas, fix_scale=False, iterations=20, device=0):
    """dvm_pose_graph_optimize (Optimizer::OptimizeEssentialGraph numerics).  Returns (S_opt[n,8], stats dict)."""
    L = lib()
    L.dvm_pose_graph_optimize.restype = C.c_int32
    L.dvm_pose_graph_optimize.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                          C.POINTER(PgStats)]
    So = np.array(S, np.float64, copy=True)
    fx = np.ascontiguousarray(fixed, np.uint8)
    e = np.zeros(len(edges_v), PG_EDGE_DTYPE)
    ev = np.asarray(edges_v)
    e["vi"] = ev[:, 0]; e["vj"] = ev[:, 1]; e["Sji"] = edges_meas
    st = PgStats()
    check(L.dvm_pose_graph_optimize(device, _p(So), _p(fx), len(So), _p(e), len(e), int(fix_scale), int(iterations), C.byref(st)))
    d = {k: getattr(st, k) for k, _ in PgStats._fields_}
    d["chi2_per_iter"] = np.array(st.chi2_per_iter[:]); d["trials_per_iter"] = np.array(st.trials_per_iter[:])
    return So, d


class PgTrialStats(C.Structure):
    _fields_ = [("nfree", C.c_int32), ("failed", C.c_int32), ("levels", C.c_int32), ("reserved", C.c_int32),
                ("chi2_before", C.c_double), ("chi2_after", C.c_double), ("scale_sum", C.c_double)]


def pose_graph_debug_trial(S, fixed, edges_v, edges_meas, fix_scale=False, lam=1e-16, device=0):
    """dvm_pose_graph_debug_trial: one LM trial of dvm_pose_graph_optimize at damping `lam`, stage by stage.  Returns a dict: e[E,7],
    J[E,2,7,7] ([error row, dof]), H[7m,7m] (lower triangle of J^T J + lam I), b[7m], x[7m] in vertex-id order of the m free vertices,
    vidx[n] (elimination position, -1 fixed), S[n,8] after oplus, chi2_before, chi2_after, scale_sum, failed, levels."""
    L = lib()
    vp, i32 = C.c_void_p, C.c_int32
    L.dvm_pose_graph_debug_trial.restype = i32
    L.dvm_pose_graph_debug_trial.argtypes = [i32, vp, vp, i32, vp, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, C.POINTER(PgTrialStats)]
    So = np.array(S, np.float64, copy=True)
    fx = np.ascontiguousarray(fixed, np.uint8)
    ed = np.zeros(len(edges_v), PG_EDGE_DTYPE)
    ev = np.asarray(edges_v)
    ed["vi"] = ev[:, 0]; ed["vj"] = ev[:, 1]; ed["Sji"] = edges_meas
    E, m = len(ed), int((fx == 0).sum())
    e = np.zeros((E, 7)); J = np.zeros((E, 2, 7, 7))
    H, b, x = (np.zeros(max(1, k))[:k] for k in (49 * m * m, 7 * m, 7 * m))     # (never a null pointer, m = 0 included)
    H = H.reshape(7 * m, 7 * m)
    vidx = np.full(len(So), -1, np.int32)
    st = PgTrialStats()
    check(L.dvm_pose_graph_debug_trial(device, _p(So), _p(fx), len(So), _p(ed), E, int(fix_scale), float(lam), _p(e), _p(J), _p(H), _p(b), _p(x),
                                       _p(vidx), C.byref(st)))
    assert st.nfree == m
    return dict(e=e, J=J, H=H, b=b, x=x, vidx=vidx, S=So, chi2_before=st.chi2_before, chi2_after=st.chi2_after, scale_sum=st.scale_sum,
                failed=int(st.failed), levels=int(st.levels), nfree=m)


TILE_FORM_FLOW, TILE_FORM_NO_PAIR, TILE_FORM_NO_DIAG_IN_LEVEL, TILE_FORM_NO_ROOT_RAW, TILE_FORM_PER_PHASE = 1, 2, 4, 8, 16
TILE_PATHS = ("none", "level_one_launch", "slices_diag_update", "diag_fused", "diag_trsm_update", "raw_root")   # DVM_TILE_PATH_*
TILE_FLOW_REFUSED = 7     # the bits of flow_refusal that forbid the flow form (bit 8: the level launches are merely preferred)


class TileSolveInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_tiles", "levels", "pair_a", "pair_b", "n_root_raw", "flow_leaves", "roots", "flow_tasks", "flow_refusal",
                                         "traced_levels", "used_pair", "used_flow", "backsolve_cols", "reserved")] + \
               [(k, C.c_int32 * 64) for k in ("level_nc", "level_ns", "level_nt", "level_path")]


def _tile_info(st):
    d = {k: int(getattr(st, k)) for k, t in TileSolveInfo._fields_ if t is C.c_int32 and k != "reserved"}
    nl = min(d["levels"], 64)
    for k in ("level_nc", "level_ns", "level_nt"):
        d[k] = [int(v) for v in getattr(st, k)[:nl]]
    d["level_path"] = [TILE_PATHS[v] for v in st.level_path[:d["traced_levels"]]]
    return d


def tile_schedule_debug(mask, workgroups=256):
    """dvm_tile_schedule_debug (host only): the schedule of a tile mask [t, t] over the tiles of unknowns, as a dict (see dvm_tile_solve_info)."""
    L = lib()
    L.dvm_tile_schedule_debug.restype = C.c_int32
    L.dvm_tile_schedule_debug.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.POINTER(TileSolveInfo)]
    m = np.ascontiguousarray(mask, np.uint8)
    assert m.ndim == 2 and m.shape[0] == m.shape[1]
    st = TileSolveInfo()
    check(L.dvm_tile_schedule_debug(len(m), _p(m), int(workgroups), C.byref(st)))
    return _tile_info(st)


def tile_solve_debug(A, b, n_blocks, dof=6, per_tile=10, kept_list=(), n_landmarks=0, mask=None, x_in=None, form=0, repeats=1, A2=None, b2=None,
                     device=0):
    """dvm_tile_solve_debug: A x = b through the tile Cholesky in the form `form` (TILE_FORM_* bits).  A[n, n] (lower triangle read), n =
    dof * n_blocks + 3 * len(kept_list).  Returns (x[repeats, dof * n_blocks + 3 * n_landmarks], fail[repeats], info dict); with A2 / b2 the
    solves of that system in between the repeats come back as info["x2"], info["fail2"]."""
    L = lib()
    vp, i32 = C.c_void_p, C.c_int32
    L.dvm_tile_solve_debug.restype = i32
    L.dvm_tile_solve_debug.argtypes = [i32, i32, i32, i32, i32, vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(TileSolveInfo)]
    kept = np.ascontiguousarray(kept_list, np.int32)
    n, xl = dof * n_blocks + 3 * len(kept), dof * n_blocks + 3 * n_landmarks
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64)
    assert A.shape == (n, n) and b.shape == (n,)
    if A2 is not None:
        A2 = np.ascontiguousarray(A2, np.float64); b2 = np.ascontiguousarray(b2, np.float64)
        assert A2.shape == (n, n) and b2.shape == (n,)
    xi = np.zeros(xl) if x_in is None else np.ascontiguousarray(x_in, np.float64)
    assert xi.shape == (xl,)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    x = np.zeros((repeats, xl)); fail = np.zeros(repeats, np.int32)
    st = TileSolveInfo()
    x2 = np.zeros((max(repeats - 1, 0), xl)); fail2 = np.zeros(max(repeats - 1, 1), np.int32)[:max(repeats - 1, 0)]
    check(L.dvm_tile_solve_debug(device, n_blocks, dof, per_tile, len(kept), _p(kept if len(kept) else None), n_landmarks, _p(A), _p(b), _p(m), _p(xi),
                                 int(form), int(repeats), _p(A2), _p(b2), _p(x), _p(fail), _p(x2 if A2 is not None else None),
                                 _p(fail2 if A2 is not None else None), C.byref(st)))
    info = _tile_info(st)
    if A2 is not None:
        info["x2"], info["fail2"] = x2, fail2
    return x, fail, info


# ---------------------------------------------------------------------------------------------------------------------
# the remaining whole ORBmatcher functions (host mirrors in dvm_slam_amd/host/orb_matcher.cpp over
# dvm_hamming_matrix / dvm_match_lists / dvm_project_search / dvm_match_triangulation).  The view structs of
# host/orb_matcher.h are mirrored as ctypes.Structure; numpy arrays referenced by a view are kept alive on the object.
class _FeatureVectorView(C.Structure):
    _fields_ = [("n", C.c_int32), ("node", C.c_void_p), ("off", C.c_void_p), ("feat", C.c_void_p)]


class _FrameView(C.Structure):
    _fields_ = [("N", C.c_int32), ("mvKeysUn", C.c_void_p), ("mDescriptors", C.c_void_p), ("mvpMapPoints", C.c_void_p),
                ("mvbOutlier", C.c_void_p), ("Tcw", C.c_float * 7), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("mnMinX", C.c_float), ("mnMaxX", C.c_float), ("mnMinY", C.c_float),
                ("mnMaxY", C.c_float), ("mvScaleFactors", C.c_void_p), ("nLevels", C.c_int32), ("dev", C.c_void_p)]


class _KeyFrameView(C.Structure):
    _fields_ = [("N", C.c_int32), ("mvKeysUn", C.c_void_p), ("mDescriptors", C.c_void_p), ("mvpMapPoints", C.c_void_p),
                ("mpBad", C.c_void_p), ("mFeatVec", _FeatureVectorView), ("Tcw", C.c_float * 7), ("Twc", C.c_float * 7),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("mnMinX", C.c_float), ("mnMaxX", C.c_float), ("mnMinY", C.c_float), ("mnMaxY", C.c_float),
                ("mvScaleFactors", C.c_void_p), ("mvLevelSigma2", C.c_void_p), ("mvInvLevelSigma2", C.c_void_p),
                ("mfLogScaleFactor", C.c_float), ("nLevels", C.c_int32)]


class _MapPointsView(C.Structure):
    _fields_ = [("n", C.c_int32), ("id", C.c_void_p), ("bad", C.c_void_p), ("pos", C.c_void_p), ("normal", C.c_void_p),
                ("min_dist", C.c_void_p), ("max_dist", C.c_void_p), ("desc", C.c_void_p)]


class _Sim3View(C.Structure):   # dvm_sim3f: Sophus::Sim3f as stored (RxSO3 quaternion x, y, z, w with |q|^2 = scale; translation)
    _fields_ = [("q", C.c_float * 4), ("t", C.c_float * 3)]


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def _fv_view(fv, keep):
    v = _FeatureVectorView()
    if fv is not None:
        arrs = [np.ascontiguousarray(fv[k], np.int32) for k in ("fv_nodes", "fv_off", "fv_feat")]
        keep.extend(arrs)
        v.n, v.node, v.off, v.feat = len(arrs[0]), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2])
    return v


def frame_view(kps, desc, bounds, scale_factors, mp=None, K=(0, 0, 0, 0), Tcw=None):
    """FrameView for the matcher mirrors; returns (struct, keepalive list).  Tcw: 7-float SE3f (qx, qy, qz, qw, t)."""
    keep = [np.ascontiguousarray(kps, KP_DTYPE), np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(scale_factors, np.float32)]
    v = _FrameView()
    v.N, v.mvKeysUn, v.mDescriptors, v.mvScaleFactors, v.nLevels = len(keep[0]), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), len(keep[2])
    if mp is not None:
        keep.append(mp)
        v.mvpMapPoints = _ptr(mp)
    v.fx, v.fy, v.cx, v.cy = (float(x) for x in K)
    v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY = (float(x) for x in bounds)
    if Tcw is not None:
        v.Tcw = (C.c_float * 7)(*np.asarray(Tcw, np.float32).reshape(7))
    return v, keep


def _pose_call(name, T, *outs):
    a = np.ascontiguousarray(T, np.float32).reshape(7)
    _hcall(name, None, C.c_void_p(a.ctypes.data), *(C.c_void_p(o.ctypes.data) for o in outs))


def se3_inverse(T):
    """Sophus::SE3f::inverse() in the product's float arithmetic (csrc/pose_f32.h); 7-float poses."""
    out = np.zeros(7, np.float32)
    _pose_call("dvmh_se3_inverse", T, out)
    return out


def pose_matrices(Tcw):
    """Frame::UpdatePoseMatrices (Frame.cc:553-559): (mRcw[3,3], mtcw, mOw) of a 7-float SE3f."""
    R = np.zeros(9, np.float32); t = np.zeros(3, np.float32); Ow = np.zeros(3, np.float32)
    _pose_call("dvmh_pose_matrices", Tcw, R, t, Ow)
    return R.reshape(3, 3), t, Ow


def sim3_to_se3(S):
    """Tcw = SE3f(Scw.rotationMatrix(), Scw.translation() / Scw.scale()), Ow = Tcw.inverse().translation() (ORBmatcher.cc:403-404)."""
    T = np.zeros(7, np.float32); Ow = np.zeros(3, np.float32)
    _pose_call("dvmh_sim3_to_se3", S, T, Ow)
    return T, Ow


def sim3_inverse(S):
    out = np.zeros(7, np.float32)
    _pose_call("dvmh_sim3_inverse", S, out)
    return out


def se3_act(T, P):
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3); out = np.zeros_like(P)
    a = np.ascontiguousarray(T, np.float32).reshape(7)
    _hcall("dvmh_se3_apply", None, C.c_void_p(a.ctypes.data), C.c_void_p(P.ctypes.data), C.c_int32(len(P)), C.c_void_p(out.ctypes.data))
    return out


def sim3_act(S, P):
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3); out = np.zeros_like(P)
    a = np.ascontiguousarray(S, np.float32).reshape(7)
    _hcall("dvmh_sim3_apply", None, C.c_void_p(a.ctypes.data), C.c_void_p(P.ctypes.data), C.c_int32(len(P)), C.c_void_p(out.ctypes.data))
    return out


def logf_shared(x):
    """The shared logf of MapPoint::PredictScale (csrc/pose_f32.h), host build."""
    return np.array([_hcall("dvmh_logf", C.c_float, C.c_float(float(v))) for v in np.asarray(x, np.float32).reshape(-1)], np.float32)


def keyframe_view(kf):
    """kf: dict(kps, desc, mp (int32, modified in place by Fuse), bad, fv, Tcw (7-float SE3f; Twc is derived as KeyFrame::SetPose
    does), K, bounds, scale_factors, level_sigma2, inv_level_sigma2, log_scale_factor); missing optional keys are NULL.
    Returns (struct, keepalive)."""
    keep = [np.ascontiguousarray(kf["kps"], KP_DTYPE), np.ascontiguousarray(kf["desc"], np.uint8)]
    v = _KeyFrameView()
    v.N, v.mvKeysUn, v.mDescriptors = len(keep[0]), _ptr(keep[0]), _ptr(keep[1])
    mp = kf.get("mp")
    if mp is not None:
        assert mp.dtype == np.int32 and mp.flags.c_contiguous
        keep.append(mp); v.mvpMapPoints = _ptr(mp)
    if kf.get("bad") is not None:
        b = np.ascontiguousarray(kf["bad"], np.uint8); keep.append(b); v.mpBad = _ptr(b)
    v.mFeatVec = _fv_view(kf.get("fv"), keep)
    if kf.get("Tcw") is not None:
        v.Tcw = (C.c_float * 7)(*np.asarray(kf["Tcw"], np.float32).reshape(7))
        v.Twc = (C.c_float * 7)(*se3_inverse(kf["Tcw"]))
    v.fx, v.fy, v.cx, v.cy = (float(x) for x in kf.get("K", (0, 0, 0, 0)))
    v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY = (float(x) for x in kf["bounds"])
    for name, key in (("mvScaleFactors", "scale_factors"), ("mvLevelSigma2", "level_sigma2"), ("mvInvLevelSigma2", "inv_level_sigma2")):
        if kf.get(key) is not None:
            a = np.ascontiguousarray(kf[key], np.float32); keep.append(a); setattr(v, name, _ptr(a)); v.nLevels = len(a)
    v.mfLogScaleFactor = float(kf.get("log_scale_factor", 0.0))
    return v, keep


def map_points_view(pts):
    """pts: dict(pos, normal, min_dist, max_dist, desc[, id, bad])."""
    keep = [np.ascontiguousarray(pts[k], np.float32) for k in ("pos", "normal", "min_dist", "max_dist")]
    keep.append(np.ascontiguousarray(pts["desc"], np.uint8))
    v = _MapPointsView()
    v.n = len(keep[2])
    v.pos, v.normal, v.min_dist, v.max_dist, v.desc = (_ptr(a) for a in keep)
    if pts.get("id") is not None:
        a = np.ascontiguousarray(pts["id"], np.int32); keep.append(a); v.id = _ptr(a)
    if pts.get("bad") is not None:
        a = np.ascontiguousarray(pts["bad"], np.uint8); keep.append(a); v.bad = _ptr(a)
    return v, keep


def _sim3_view(S):
    S = np.asarray(S, np.float32).reshape(7)
    v = _Sim3View()
    v.q = (C.c_float * 4)(*S[:4]); v.t = (C.c_float * 3)(*S[4:])
    return v


def _hcall(name, restype, *args):
    fn = getattr(host_lib(), name)
    fn.restype = restype
    fn.argtypes = None
    return fn(*args)


def search_for_initialization(F1, F2, prev_matched, window=100, nnratio=0.9, check_ori=True, device=0):
    """dvm_host::ORBmatcher::SearchForInitialization (ORBmatcher.cc:605-707).  F1 / F2 = frame_view() results.
    Returns (nmatches, vnMatches12, vbPrevMatched updated)."""
    pm = np.array(prev_matched, np.float32, copy=True).reshape(-1, 2)
    m = np.zeros(max(F1[0].N, 1), np.int32)
    n = _hcall("dvmh_search_for_initialization", C.c_int32, C.c_int32(device), C.byref(F1[0]), C.byref(F2[0]), C.c_void_p(pm.ctypes.data),
               C.c_void_p(m.ctypes.data), C.c_int32(int(window)), C.c_float(nnratio), C.c_int32(int(check_ori)))
    check(min(n, 0))
    return n, m[:F1[0].N], pm


def search_by_bow_kf_frame(KF, F, fv_f, nnratio=0.7, check_ori=True, device=0):
    """SearchByBoW(KF, F, vpMapPointMatches) (:214-393).  Returns (nmatches, matches[F.N], #host re-queries)."""
    keep = []
    fv = _fv_view(fv_f, keep)
    m = np.zeros(max(F[0].N, 1), np.int32); rq = C.c_int32(0)
    n = _hcall("dvmh_search_by_bow_kf_frame", C.c_int32, C.c_int32(device), C.byref(KF[0]), C.byref(F[0]), C.byref(fv), C.c_float(nnratio),
               C.c_int32(int(check_ori)), C.c_void_p(m.ctypes.data), C.byref(rq))
    check(min(n, 0))
    return n, m[:F[0].N], rq.value


def search_by_bow_kf_kf(KF1, KF2, nnratio=0.8, check_ori=True, device=0):
    """SearchByBoW(KF1, KF2, vpMatches12) (:709-834).  Returns (nmatches, matches12[KF1.N], #host re-queries)."""
    m = np.zeros(max(KF1[0].N, 1), np.int32); rq = C.c_int32(0)
    n = _hcall("dvmh_search_by_bow_kf_kf", C.c_int32, C.c_int32(device), C.byref(KF1[0]), C.byref(KF2[0]), C.c_float(nnratio),
               C.c_int32(int(check_ori)), C.c_void_p(m.ctypes.data), C.byref(rq))
    check(min(n, 0))
    return n, m[:KF1[0].N], rq.value


def triangulation_geometry(KF1, KF2):
    R12 = np.zeros(9, np.float32); t12 = np.zeros(3, np.float32); ep = np.zeros(2, np.float32); F12 = np.zeros(9, np.float32)
    _hcall("dvmh_triangulation_geometry", None, C.byref(KF1[0]), C.byref(KF2[0]), *(C.c_void_p(a.ctypes.data) for a in (R12, t12, ep, F12)))
    return R12, t12, ep, F12


def search_for_triangulation(KF1, KF2, coarse=False, check_ori=True, device=0):
    """SearchForTriangulation (:836-1058, mono).  Returns (nmatches, pairs[nmatches, 2])."""
    pairs = np.zeros((max(KF1[0].N, 1), 2), np.int32)
    n = _hcall("dvmh_search_for_triangulation", C.c_int32, C.c_int32(device), C.byref(KF1[0]), C.byref(KF2[0]), C.c_int32(int(coarse)),
               C.c_int32(int(check_ori)), C.c_void_p(pairs.ctypes.data))
    check(min(n, 0))
    return n, pairs[:n]


def triangulation_geometry_cam(KF1, KF2, model1, model2):
    """dvmh_triangulation_geometry_cam: R12, t12, the epipole through model2, F12 (Pinhole's formula on p[0..3])."""
    R12 = np.zeros(9, np.float32); t12 = np.zeros(3, np.float32); ep = np.zeros(2, np.float32); F12 = np.zeros(9, np.float32)
    check(_hcall("dvmh_triangulation_geometry_cam", C.c_int32, C.byref(KF1[0]), C.byref(KF2[0]), _model_ref(model1), _model_ref(model2),
                 *(C.c_void_p(a.ctypes.data) for a in (R12, t12, ep, F12))))
    return R12, t12, ep, F12


def search_for_triangulation_cam(KF1, KF2, model1, model2, coarse=False, check_ori=True, device=0):
    """dvmh_search_for_triangulation_cam: SearchForTriangulation on a CameraModel per keyframe.  Returns (nmatches, pairs[nmatches, 2])."""
    pairs = np.zeros((max(KF1[0].N, 1), 2), np.int32)
    n = _hcall("dvmh_search_for_triangulation_cam", C.c_int32, C.c_int32(device), C.byref(KF1[0]), C.byref(KF2[0]), _model_ref(model1), _model_ref(model2),
               C.c_int32(int(coarse)), C.c_int32(int(check_ori)), C.c_void_p(pairs.ctypes.data))
    check(min(n, 0))
    return n, pairs[:n]


def fuse(KF, P, in_kf, th, device=0):
    """Fuse(KF, vpMapPoints, th) search part (:1060-1213).  Returns (count, vBestIdx)."""
    bi = np.zeros(max(P[0].n, 1), np.int32)
    ik = None if in_kf is None else np.ascontiguousarray(in_kf, np.uint8)
    n = _hcall("dvmh_fuse", C.c_int32, C.c_int32(device), C.byref(KF[0]), C.byref(P[0]), None if ik is None else C.c_void_p(ik.ctypes.data),
               C.c_float(th), C.c_void_p(bi.ctypes.data))
    check(min(n, 0))
    return n, bi[:P[0].n]


def fuse_sim3(KF, Scw, P, th, device=0):
    """Fuse(KF, Scw, vpPoints, th, vpReplacePoint) (:1236-1345); Scw: 7-float Sim3f; KF's mp array is updated in place.
    Returns (nFused, replace)."""
    S = _sim3_view(Scw)
    rep = np.zeros(max(P[0].n, 1), np.int32)
    n = _hcall("dvmh_fuse_sim3", C.c_int32, C.c_int32(device), C.byref(KF[0]), C.byref(S), C.byref(P[0]), C.c_float(th), C.c_void_p(rep.ctypes.data))
    check(min(n, 0))
    return n, rep[:P[0].n]


def search_by_projection_sim3(KF, Scw, P, matched, th, ratio_hamming=1.0, device=0, point_kf=None, matched_kf=None):
    """SearchByProjection(KF, Scw, vpPoints, vpMatched, th, ratioHamming) (:395-496); with point_kf / matched_kf the overload
    that also fills vpMatchedKF (:498-603).  Scw: 7-float Sim3f.  Returns (nmatches, vpMatched, #re-queries[, vpMatchedKF])."""
    S = _sim3_view(Scw)
    m = np.array(matched, np.int32, copy=True); rq = C.c_int32(0)
    pk = None if point_kf is None else np.ascontiguousarray(point_kf, np.int32)
    mk = None if matched_kf is None else np.array(matched_kf, np.int32, copy=True)
    n = _hcall("dvmh_search_by_projection_sim3", C.c_int32, C.c_int32(device), C.byref(KF[0]), C.byref(S), C.byref(P[0]),
               None if pk is None else C.c_void_p(pk.ctypes.data), C.c_void_p(m.ctypes.data),
               None if mk is None else C.c_void_p(mk.ctypes.data), C.c_int32(int(th)), C.c_float(ratio_hamming), C.byref(rq))
    check(min(n, 0))
    return (n, m, rq.value) if mk is None else (n, m, rq.value, mk)


def search_by_projection_reloc(Cur, KF, P, already, th, orb_dist, check_ori=True, device=0):
    """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1750-1860).  Cur = frame_view(...) built with its mp
    array (updated in place) and pose set on the struct.  Returns (nmatches, #host re-queries)."""
    al = np.sort(np.ascontiguousarray(already, np.int32)); rq = C.c_int32(0)
    n = _hcall("dvmh_search_by_projection_reloc", C.c_int32, C.c_int32(device), C.byref(Cur[0]), C.byref(KF[0]), C.byref(P[0]),
               C.c_void_p(al.ctypes.data) if len(al) else None, C.c_int32(len(al)), C.c_float(th), C.c_int32(int(orb_dist)),
               C.c_int32(int(check_ori)), C.byref(rq))
    check(min(n, 0))
    return n, rq.value


def search_by_sim3(KF1, KF2, P1, P2, matches12, idx_in_kf2, S12, th, device=0):
    """SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (:1347-1551).  S12: 7-float Sim3f.  Returns (nFound, vpMatches12 updated)."""
    S = _sim3_view(S12)
    m = np.array(matches12, np.int32, copy=True)
    ix = None if idx_in_kf2 is None else np.ascontiguousarray(idx_in_kf2, np.int32)
    n = _hcall("dvmh_search_by_sim3", C.c_int32, C.c_int32(device), C.byref(KF1[0]), C.byref(KF2[0]), C.byref(P1[0]), C.byref(P2[0]),
               C.c_void_p(m.ctypes.data), None if ix is None else C.c_void_p(ix.ctypes.data), C.byref(S), C.c_float(th))
    check(min(n, 0))
    return n, m


class _KfCamera(C.Structure):   # == dvm_kf_camera
    _fields_ = [("Tcw", C.c_float * 7), ("Ow", C.c_float * 3), ("K", C.c_float * 4), ("b", C.c_float * 4),
                ("lsf", C.c_float), ("nl", C.c_int32), ("sim3_pair", C.c_int32), ("S2", C.c_float * 7)]


def _project_search_call(fn, grid, cam, model_args, pts, th, scale_factors, skip, gate_inv_sigma2, gate, valid):
    """dvm_project_search / dvm_project_search_cam on a FrameGrid slot 0: packs the camera dict and the points; model_args goes behind cam."""
    sf = np.ascontiguousarray(scale_factors, np.float32)
    c = _KfCamera()
    c.Tcw = (C.c_float * 7)(*np.asarray(cam["Tcw"], np.float32).reshape(7))
    c.sim3_pair = int(cam.get("sim3_pair", 0))
    if cam.get("S2") is not None:
        c.S2 = (C.c_float * 7)(*np.asarray(cam["S2"], np.float32).reshape(7))
    c.Ow = (C.c_float * 3)(*np.asarray(cam["Ow"], np.float32)); c.K = (C.c_float * 4)(*np.asarray(cam.get("K", (0, 0, 0, 0)), np.float32))
    c.b = (C.c_float * 4)(*np.asarray(cam["bounds"], np.float32)); c.lsf = float(cam["log_scale_factor"]); c.nl = len(sf)
    P, keep = map_points_view(pts)
    n = P.n
    out = np.zeros(max(n, 1), MATCH_DTYPE); proj = np.zeros(max(n, 1), np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("level", "<i4")]))
    sk = None
    if skip is not None:
        sk = np.zeros(grid.capacity, np.uint8); sk[:len(skip)] = skip
    gi = None if gate_inv_sigma2 is None else np.ascontiguousarray(gate_inv_sigma2, np.float32)
    va = None if valid is None else np.ascontiguousarray(valid, np.uint8)
    fn.restype = C.c_int32; fn.argtypes = None
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    check(fn(grid.h, C.c_int32(0), vp(sk), C.byref(c), *model_args, C.c_void_p(P.pos), C.c_void_p(P.normal), C.c_void_p(P.min_dist), C.c_void_p(P.max_dist),
             C.c_void_p(P.desc), vp(va), C.c_int32(n), C.c_float(th), vp(sf), vp(gi), C.c_double(gate), vp(out), vp(proj), C.c_int32(0), None))
    return out[:n], proj[:n]


def project_search(grid, cam, pts, th, scale_factors, skip=None, gate_inv_sigma2=None, gate=5.99, valid=None):
    """dvm_project_search on a FrameGrid slot 0.  cam: dict(Tcw (7-float SE3f), Ow, K, bounds, log_scale_factor[, sim3_pair, S2]).
    Returns (matches, proj)."""
    return _project_search_call(lib().dvm_project_search, grid, cam, (), pts, th, scale_factors, skip, gate_inv_sigma2, gate, valid)


def project_search_cam(grid, cam, model, pts, th, scale_factors, skip=None, gate_inv_sigma2=None, gate=5.99, valid=None):
    """dvm_project_search_cam: project_search with the projection of a CameraModel (cam["K"] is not read and may be absent)."""
    return _project_search_call(lib().dvm_project_search_cam, grid, cam, (None if model is None else C.byref(model),), pts, th, scale_factors, skip,
                                gate_inv_sigma2, gate, valid)


def bowdb_query_raw(bows, q_ids, q_vals, erase=(), device=0):
    """dvm_bowdb_* directly: store `bows` (list of (ids, vals)), erase some slots, query.  Returns (common, first_word, score)."""
    L = lib()
    h = C.c_void_p()
    L.dvm_bowdb_create.restype = C.c_int32; L.dvm_bowdb_create.argtypes = [C.c_int32, C.c_void_p]
    check(L.dvm_bowdb_create(device, C.byref(h)))
    try:
        for ids, vals in bows:
            i = np.ascontiguousarray(ids, np.int32); v = np.ascontiguousarray(vals, np.float64)
            slot = C.c_int32(-1)
            L.dvm_bowdb_add.restype = C.c_int32; L.dvm_bowdb_add.argtypes = None
            check(L.dvm_bowdb_add(h, C.c_void_p(i.ctypes.data) if len(i) else None, C.c_void_p(v.ctypes.data) if len(v) else None,
                                  C.c_int32(len(i)), C.byref(slot)))
        for s in erase:
            L.dvm_bowdb_erase.restype = C.c_int32; L.dvm_bowdb_erase.argtypes = None
            check(L.dvm_bowdb_erase(h, C.c_int32(int(s))))
        n = len(bows)
        qi = np.ascontiguousarray(q_ids, np.int32); qv = np.ascontiguousarray(q_vals, np.float64)
        common = np.zeros(n, np.int32); first = np.zeros(n, np.int32); score = np.zeros(n, np.float32)
        L.dvm_bowdb_query.restype = C.c_int32; L.dvm_bowdb_query.argtypes = None
        check(L.dvm_bowdb_query(h, C.c_void_p(qi.ctypes.data) if len(qi) else None, C.c_void_p(qv.ctypes.data) if len(qv) else None,
                                C.c_int32(len(qi)), C.c_void_p(common.ctypes.data), C.c_void_p(first.ctypes.data), C.c_void_p(score.ctypes.data)))
        return common, first, score
    finally:
        L.dvm_bowdb_destroy.restype = None; L.dvm_bowdb_destroy.argtypes = [C.c_void_p]
        L.dvm_bowdb_destroy(h)


class BowDb:
    """dvm_bowdb_* handle (tests): add / erase / query / stats on one store."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.L.dvm_bowdb_create.restype = C.c_int32; self.L.dvm_bowdb_create.argtypes = [C.c_int32, C.c_void_p]
        check(self.L.dvm_bowdb_create(device, C.byref(self.h)))
        self.n = 0

    def add(self, ids, vals):
        i = np.ascontiguousarray(ids, np.int32); v = np.ascontiguousarray(vals, np.float64)
        slot = C.c_int32(-1)
        self.L.dvm_bowdb_add.restype = C.c_int32; self.L.dvm_bowdb_add.argtypes = None
        check(self.L.dvm_bowdb_add(self.h, C.c_void_p(i.ctypes.data) if len(i) else None, C.c_void_p(v.ctypes.data) if len(v) else None,
                                   C.c_int32(len(i)), C.byref(slot)))
        self.n += 1
        return slot.value

    def erase(self, slot):
        self.L.dvm_bowdb_erase.restype = C.c_int32; self.L.dvm_bowdb_erase.argtypes = None
        check(self.L.dvm_bowdb_erase(self.h, C.c_int32(int(slot))))

    def query(self, q_ids, q_vals):
        qi = np.ascontiguousarray(q_ids, np.int32); qv = np.ascontiguousarray(q_vals, np.float64)
        common = np.zeros(self.n, np.int32); first = np.zeros(self.n, np.int32); score = np.zeros(self.n, np.float32)
        self.L.dvm_bowdb_query.restype = C.c_int32; self.L.dvm_bowdb_query.argtypes = None
        check(self.L.dvm_bowdb_query(self.h, C.c_void_p(qi.ctypes.data) if len(qi) else None, C.c_void_p(qv.ctypes.data) if len(qv) else None,
                                     C.c_int32(len(qi)), C.c_void_p(common.ctypes.data), C.c_void_p(first.ctypes.data), C.c_void_p(score.ctypes.data)))
        return common, first, score

    def stats(self):
        out = np.zeros(4, np.int64)
        self.L.dvm_bowdb_stats.restype = C.c_int32; self.L.dvm_bowdb_stats.argtypes = [C.c_void_p, C.c_void_p]
        check(self.L.dvm_bowdb_stats(self.h, _p(out)))
        return dict(slots=int(out[0]), live=int(out[1]), words=int(out[2]), capacity=int(out[3]))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.dvm_bowdb_destroy.restype = None; self.L.dvm_bowdb_destroy.argtypes = [C.c_void_p]
            self.L.dvm_bowdb_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close


class HostKeyFrameDatabase:
    """dvm_host::KeyFrameDatabase (host/keyframe_database.cpp over dvm_bowdb_*): add / erase / CalculateMergeScore /
    DetectMergePossibility / DetectNBestCandidates on keyframe slots (reference KeyFrameDatabase.cc:43-70,555-808)."""
    PREFIX = "dvmh_kfdb_"

    def _lib(self):
        return host_lib()

    def __init__(self, device=0):
        f = host_lib().dvmh_kfdb_create; f.restype = C.c_void_p; f.argtypes = [C.c_int32]
        self.h = C.c_void_p(f(device))
        if not self.h.value:
            raise DvmError(-5, lib().dvm_last_error().decode(errors="replace"))

    def _f(self, name, restype=None):
        f = getattr(self._lib(), self.PREFIX + name); f.restype = restype; f.argtypes = None
        return f

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self._f("destroy")(self.h); self.h = C.c_void_p()

    __del__ = close

    @staticmethod
    def _bow(ids, vals):
        return np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vals, np.float64)

    def add(self, ids, vals, map_id, uuid, mn_id):
        i, v = self._bow(ids, vals)
        return self._f("add", C.c_int32)(self.h, _p(i), _p(v), C.c_int32(len(i)), C.c_int32(map_id), C.c_uint64(uuid), C.c_int64(mn_id))

    def erase(self, slot): self._f("erase")(self.h, C.c_int32(slot))
    def set_bad(self, slot, bad): self._f("set_bad")(self.h, C.c_int32(slot), C.c_int32(int(bad)))
    def set_map_bad(self, map_id, bad): self._f("set_map_bad")(self.h, C.c_int32(map_id), C.c_int32(int(bad)))

    def set_neighbours(self, slot, neigh):
        a = np.ascontiguousarray(neigh, np.int32)
        self._f("set_neighbours")(self.h, C.c_int32(slot), _p(a) if len(a) else None, C.c_int32(len(a)))

    def set_connected(self, slot, conn):
        a = np.ascontiguousarray(conn, np.int32)
        self._f("set_connected")(self.h, C.c_int32(slot), _p(a) if len(a) else None, C.c_int32(len(a)))

    def state(self, slot):
        q = C.c_uint64(0); w = C.c_int32(0); s = C.c_float(0)
        self._f("get_state")(self.h, C.c_int32(slot), C.byref(q), C.byref(w), C.byref(s))
        return q.value, w.value, s.value

    def merge_score(self, ids, vals, key_frame_id, map_id, score=0.0):
        i, v = self._bow(ids, vals)
        sc = C.c_float(score); best = C.c_int32(-1)
        self._f("merge_score", C.c_int32)(self.h, _p(i), _p(v), C.c_int32(len(i)), C.c_uint64(key_frame_id), C.c_int32(map_id), C.byref(sc), C.byref(best))
        return sc.value, best.value

    def detect_merge_possibility(self, ids, vals, uuid, map_id):
        i, v = self._bow(ids, vals)
        best = C.c_int32(-1); sc = C.c_float(0); base = C.c_float(0)
        r = self._f("detect_merge_possibility", C.c_int32)(self.h, _p(i), _p(v), C.c_int32(len(i)), C.c_uint64(uuid), C.c_int32(map_id), C.byref(best),
                                                           C.byref(sc), C.byref(base))
        if r < 0:
            check(r)
        return r, best.value, sc.value, base.value

    def detect_reloc(self, ids, vals, frame_id, map_id, cap=4096):
        """DetectRelocalizationCandidates(F, pMap): candidate slots in the reference's order."""
        i, v = self._bow(ids, vals)
        out = np.zeros(cap, np.int32); n = C.c_int32(0)
        self._f("detect_reloc", C.c_int32)(self.h, _p(i), _p(v), C.c_int32(len(i)), C.c_uint64(frame_id), C.c_int32(map_id), _p(out), C.byref(n))
        return out[:n.value].copy()

    def reloc_state(self, slot):
        q = C.c_uint64(0); w = C.c_int32(0); sc = C.c_float(0)
        self._f("get_reloc_state")(self.h, C.c_int32(slot), C.byref(q), C.byref(w), C.byref(sc))
        return q.value, w.value, sc.value

    def detect_n_best(self, slot, n_num):
        lo = np.zeros(max(n_num, 1), np.int32); me = np.zeros(max(n_num, 1), np.int32)
        nl = C.c_int32(0); nm = C.c_int32(0)
        self._f("detect_n_best", C.c_int32)(self.h, C.c_int32(slot), C.c_int32(n_num), _p(lo), C.byref(nl), _p(me), C.byref(nm))
        return lo[:nl.value].copy(), me[:nm.value].copy()


# ---------------------------------------------------------------------------------------------------------------------
# LocalMapping::CreateNewMapPoints as one device chain (dvm_create_new_map_points / dvmh_create_new_map_points).  Keyframes are the
# dicts keyframe_view() takes (kps, desc, mp, fv, Tcw, K, bounds, scale_factors, level_sigma2).
class _NpKeyFrame(C.Structure):   # == dvm_np_keyframe
    _fields_ = [("n", C.c_int32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("mp", C.c_void_p), ("fv_n", C.c_int32), ("fv_node", C.c_void_p),
                ("fv_off", C.c_void_p), ("fv_feat", C.c_void_p), ("Tcw", C.c_float * 7), ("Twc", C.c_float * 7), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("scale_factors", C.c_void_p),
                ("level_sigma2", C.c_void_p), ("n_levels", C.c_int32)]


class _NpNeighbour(C.Structure):   # == dvm_np_neighbour
    _fields_ = [("kf", _NpKeyFrame), ("median_depth", C.c_float), ("ep", C.c_float * 2), ("F12", C.c_float * 9)]


class _NpParams(C.Structure):   # == dvm_np_params
    _fields_ = [("cos_parallax_max", C.c_double), ("ratio_factor", C.c_float), ("th_far", C.c_float), ("far_points", C.c_int32),
                ("coarse", C.c_int32), ("check_ori", C.c_int32), ("monocular", C.c_int32)]


class _NpOut(C.Structure):   # == dvm_np_out
    _fields_ = [("nb_status", C.c_void_p), ("nb_matches", C.c_void_p), ("pair_off", C.c_void_p), ("pairs", C.c_void_p), ("status", C.c_void_p),
                ("x3D", C.c_void_p), ("new_point", C.c_void_p), ("record_cap", C.c_int32)]


def _np_params(cur, coarse=False, check_ori=False, cos_parallax_max=0.9998, ratio_factor=None, far_points=False, th_far=0.0, monocular=1):
    """check_ori = False is what CreateNewMapPoints' matcher has (ORBmatcher(0.6f, false), LocalMapping.cc:467); ratio_factor defaults to
    1.5f * the current keyframe's mfScaleFactor (:483)."""
    p = _NpParams()
    if ratio_factor is None:
        ratio_factor = np.float32(1.5) * np.float32(np.asarray(cur["scale_factors"], np.float32)[1])
    p.cos_parallax_max, p.ratio_factor, p.th_far = float(cos_parallax_max), float(ratio_factor), float(th_far)
    p.far_points, p.coarse, p.check_ori, p.monocular = int(far_points), int(coarse), int(check_ori), int(monocular)
    return p


class _NpResult:
    """The caller memory of dvm_np_out, and the dict handed back."""

    def __init__(self, n1, n_nb, record_cap):
        self.nb_status = np.zeros(max(n_nb, 1), np.int32); self.nb_matches = np.zeros(max(n_nb, 1), np.int32)
        self.pair_off = np.zeros(n_nb + 1, np.int32)
        self.pairs = np.zeros((max(record_cap, 1), 2), np.int32); self.status = np.zeros(max(record_cap, 1), np.int32)
        self.x3D = np.zeros((max(record_cap, 1), 3), np.float32); self.new_point = np.zeros(max(n1, 1), np.int32)
        self.n1, self.n_nb = n1, n_nb
        o = self.out = _NpOut()
        o.nb_status, o.nb_matches, o.pair_off, o.pairs = (a.ctypes.data for a in (self.nb_status, self.nb_matches, self.pair_off, self.pairs))
        o.status, o.x3D, o.new_point, o.record_cap = self.status.ctypes.data, self.x3D.ctypes.data, self.new_point.ctypes.data, int(record_cap)

    def result(self):
        m = int(self.pair_off[self.n_nb])
        return dict(nb_status=self.nb_status[:self.n_nb].copy(), nb_matches=self.nb_matches[:self.n_nb].copy(), pair_off=self.pair_off.copy(),
                    pairs=self.pairs[:m].copy(), status=self.status[:m].copy(), x3D=self.x3D[:m].copy(), new_point=self.new_point[:self.n1].copy())


def _np_record_cap(cur, n_nb, record_cap):
    return int(record_cap) if record_cap is not None else int((np.asarray(cur["mp"]) < 0).sum()) * n_nb


class _Chain:
    """A device-chain handle over <prefix>_create / _destroy / _reserve / _profiling / _last_kernel_ms, bound once at construction."""

    def __init__(self, prefix, n_kernel_ms, device=0):
        self.L = lib()
        vp, i32 = C.c_void_p, C.c_int32
        create, self._destroy, self._reserve_fn, self._profiling, self._last_ms = (
            getattr(self.L, f"{prefix}_{name}") for name in ("create", "destroy", "reserve", "profiling", "last_kernel_ms"))
        create.argtypes = [i32, C.POINTER(vp)]
        self._destroy.argtypes = [vp]; self._destroy.restype = None
        self._reserve_fn.argtypes = [vp, i32, i32, i32]
        self._profiling.argtypes = [vp, i32]
        self._last_ms.argtypes = [vp, vp]
        self._n_kernel_ms = n_kernel_ms
        self.h = vp()
        check(create(device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self._destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _reserve(self, a, b, c):
        check(self._reserve_fn(self.h, int(a), int(b), int(c)))

    def profiling(self, enable=True):
        check(self._profiling(self.h, int(enable)))

    def _last_kernel_ms(self):
        ms = np.zeros(self._n_kernel_ms, np.float32)
        check(self._last_ms(self.h, _p(ms)))
        return ms


class NewPoints(_Chain):
    """dvm_new_points: LocalMapping::CreateNewMapPoints for all neighbour keyframes as one device chain."""

    def __init__(self, device=0):
        super().__init__("dvm_new_points", 3, device)
        vp = C.c_void_p
        self.L.dvm_create_new_map_points.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
        self.L.dvm_create_new_map_points_cam.argtypes = [vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]

    def reserve(self, max_kf1_keypoints, max_neighbours, max_total_neighbour_keypoints):
        self._reserve(max_kf1_keypoints, max_neighbours, max_total_neighbour_keypoints)

    def last_kernel_ms(self):
        """(search, geometry, settle) milliseconds of the last call that ran with profiling on."""
        return self._last_kernel_ms()

    @staticmethod
    def _keyframe(kf, keep):
        """dict -> dvm_np_keyframe; Twc / Ow as KeyFrame::SetPose derives them (Ow = Twc's translation)."""
        v, k = keyframe_view(kf)
        keep.append(k)
        s = _NpKeyFrame()
        s.n, s.kps, s.desc, s.mp = v.N, v.mvKeysUn, v.mDescriptors, v.mvpMapPoints
        s.fv_n, s.fv_node, s.fv_off, s.fv_feat = v.mFeatVec.n, v.mFeatVec.node, v.mFeatVec.off, v.mFeatVec.feat
        s.Tcw = v.Tcw; s.Twc = v.Twc
        s.Ow = (C.c_float * 3)(*v.Twc[4:7])
        s.fx, s.fy, s.cx, s.cy = v.fx, v.fy, v.cx, v.cy
        s.scale_factors, s.level_sigma2, s.n_levels = v.mvScaleFactors, v.mvLevelSigma2, v.nLevels
        return s, v

    def prepare(self, cur, neighbours, median_depth, record_cap=None, **params):
        """The argument structs of a call built once (views, pair geometry, result arrays): returns run() -> result dict, for a caller
        that repeats the call on the same keyframes (a timing loop).  The arrays of `cur` / `neighbours` are read in place at run()."""
        keep = []
        c, cv = self._keyframe(cur, keep)
        n_nb = len(neighbours)
        nbs = (_NpNeighbour * max(n_nb, 1))()
        for j, kf in enumerate(neighbours):
            s, v = self._keyframe(kf, keep)
            nbs[j].kf = s
            nbs[j].median_depth = float(median_depth[j])
            _, _, ep, F12 = triangulation_geometry((cv, None), (v, None))
            nbs[j].ep = (C.c_float * 2)(*ep); nbs[j].F12 = (C.c_float * 9)(*F12)
        p = _np_params(cur, **params)
        R = _NpResult(c.n, n_nb, _np_record_cap(cur, n_nb, record_cap))

        def run():
            keep  # noqa: B018 (the views' arrays live as long as the closure)
            check(self.L.dvm_create_new_map_points(self.h, C.addressof(c), n_nb, C.addressof(nbs), C.addressof(p), C.addressof(R.out)))
            return R.result()
        return run

    def prepare_cam(self, cur, neighbours, median_depth, cur_model, nb_models, record_cap=None, **params):
        """prepare() for dvm_create_new_map_points_cam: cur_model / nb_models[j] = the CameraModel of the current keyframe / neighbour j
        (None is passed on as NULL).  The epipole goes through the neighbour's model; the relative poses come from dvm_pair_pose_set."""
        keep = []
        c, cv = self._keyframe(cur, keep)
        n_nb = len(neighbours)
        nbs = (_NpNeighbour * max(n_nb, 1))()
        poses = (PairPose * max(n_nb, 1))()
        models = (CameraModel * max(n_nb, 1))()
        have_models = cur_model is not None and nb_models is not None and all(m is not None for m in nb_models)
        for j, kf in enumerate(neighbours):
            s, v = self._keyframe(kf, keep)
            nbs[j].kf = s
            nbs[j].median_depth = float(median_depth[j])
            if have_models:
                models[j] = nb_models[j]
                ok = cur_model.model == nb_models[j].model and cur_model.model in (0, 1) and all(m.p[0] != 0 and m.p[1] != 0 for m in (cur_model, nb_models[j]))
                if ok:
                    R12, t12, ep, F12 = triangulation_geometry_cam((cv, None), (v, None), cur_model, nb_models[j])
                    nbs[j].ep = (C.c_float * 2)(*ep); nbs[j].F12 = (C.c_float * 9)(*F12)
                    poses[j] = pair_pose(R12, t12)
        p = _np_params(cur, **params)
        R = _NpResult(c.n, n_nb, _np_record_cap(cur, n_nb, record_cap))

        def run():
            keep  # noqa: B018 (the views' arrays live as long as the closure)
            check(self.L.dvm_create_new_map_points_cam(self.h, C.addressof(c), None if cur_model is None else C.addressof(cur_model), n_nb, C.addressof(nbs),
                                                       C.addressof(models) if have_models or cur_model is None else None, C.addressof(poses), C.addressof(p),
                                                       C.addressof(R.out)))
            return R.result()
        return run

    @staticmethod
    def _keyframe_resident(slot, kf, keep):
        """(dvm_np_keyframe_resident, view) of keyframe dict `kf` living in store slot `slot`: mp and the pose travel, the rest is the slot's."""
        v, k = keyframe_view(kf)
        keep.append(k)
        s = _NpKeyFrameResident()
        s.slot, s.mp = int(slot), v.mvpMapPoints
        s.Tcw = v.Tcw; s.Twc = v.Twc
        s.Ow = (C.c_float * 3)(*v.Twc[4:7])
        return s, v

    def prepare_resident(self, store, cur_slot, cur, nb_slots, neighbours, median_depth, cur_model=None, nb_models=None, record_cap=None, **params):
        """prepare() for dvm_create_new_map_points_resident: `cur` / neighbours[j] are the keyframe dicts that were put to cur_slot /
        nb_slots[j] of `store` (a KeyframeStore).  Of a dict the call sends mp and the pose; its intrinsics and poses also give the pair
        geometry (ep, F12; with cur_model / nb_models the rules of prepare_cam).  mp is read in place at run()."""
        keep = []
        c, cv = self._keyframe_resident(cur_slot, cur, keep)
        n_nb = len(neighbours)
        assert len(nb_slots) == n_nb
        nbs = (_NpNeighbourResident * max(n_nb, 1))()
        poses = (PairPose * max(n_nb, 1))()
        models = (CameraModel * max(n_nb, 1))()
        for j, kf in enumerate(neighbours):
            s, v = self._keyframe_resident(nb_slots[j], kf, keep)
            nbs[j].kf = s
            nbs[j].median_depth = float(median_depth[j])
            if cur_model is None:
                _, _, ep, F12 = triangulation_geometry((cv, None), (v, None))
            else:
                models[j] = nb_models[j]
                R12, t12, ep, F12 = triangulation_geometry_cam((cv, None), (v, None), cur_model, nb_models[j])
                poses[j] = pair_pose(R12, t12)
            nbs[j].ep = (C.c_float * 2)(*ep); nbs[j].F12 = (C.c_float * 9)(*F12)
        p = _np_params(cur, **params)
        R = _NpResult(len(cur["kps"]), n_nb, _np_record_cap(cur, n_nb, record_cap))
        fn = self.L.dvm_create_new_map_points_resident
        vp = C.c_void_p
        fn.restype = C.c_int32; fn.argtypes = [vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]

        def run():
            keep  # noqa: B018 (the views' arrays live as long as the closure)
            check(fn(self.h, store.h, C.addressof(c), None if cur_model is None else C.addressof(cur_model), n_nb, C.addressof(nbs),
                     None if cur_model is None else C.addressof(models), None if cur_model is None else C.addressof(poses), C.addressof(p),
                     C.addressof(R.out)))
            return R.result()
        return run

    def create_new_map_points_resident(self, store, cur_slot, cur, nb_slots, neighbours, median_depth, cur_model=None, nb_models=None, record_cap=None,
                                       **params):
        """dvm_create_new_map_points_resident; arguments as prepare_resident, result as create_new_map_points."""
        return self.prepare_resident(store, cur_slot, cur, nb_slots, neighbours, median_depth, cur_model, nb_models, record_cap=record_cap, **params)()

    def last_upload_bytes(self):
        """The host-to-device bytes queued by the last call that reached the device, resident or not."""
        a = C.c_int64(0)
        fn = self.L.dvm_new_points_last_upload_bytes
        fn.restype = C.c_int32; fn.argtypes = [C.c_void_p, C.c_void_p]
        check(fn(self.h, C.byref(a)))
        return a.value

    def create_new_map_points_cam(self, cur, neighbours, median_depth, cur_model, nb_models, record_cap=None, **params):
        """dvm_create_new_map_points_cam; arguments as prepare_cam, result as create_new_map_points."""
        return self.prepare_cam(cur, neighbours, median_depth, cur_model, nb_models, record_cap=record_cap, **params)()

    def create_new_map_points(self, cur, neighbours, median_depth, record_cap=None, **params):
        """cur / neighbours: keyframe dicts; median_depth[j] = ComputeSceneMedianDepth(2) of neighbour j.  params: coarse, check_ori,
        cos_parallax_max, ratio_factor, far_points, th_far, monocular.  Returns dict(nb_status, nb_matches, pair_off, pairs[m, 2],
        status[m], x3D[m, 3], new_point[n1])."""
        return self.prepare(cur, neighbours, median_depth, record_cap=record_cap, **params)()


def create_new_map_points(cur, neighbours, median_depth, device=0, record_cap=None, **params):
    """dvmh_create_new_map_points: the host entry (pair geometry, camera centres and the calling thread's chain handle inside).
    Arguments and result as NewPoints.create_new_map_points."""
    keep = []
    cv, k = keyframe_view(cur); keep.append(k)
    n_nb = len(neighbours)
    views = (_KeyFrameView * max(n_nb, 1))()
    for j, kf in enumerate(neighbours):
        v, k = keyframe_view(kf); keep.append(k)
        views[j] = v
    md = np.ascontiguousarray(median_depth, np.float32)
    p = _np_params(cur, **params)
    R = _NpResult(cv.N, n_nb, _np_record_cap(cur, n_nb, record_cap))
    rc = _hcall("dvmh_create_new_map_points", C.c_int32, C.c_int32(device), C.byref(cv), C.c_int32(n_nb), C.byref(views), C.c_void_p(md.ctypes.data if md.size else None),
                C.byref(p), C.byref(R.out))
    check(rc)
    return R.result()


def create_new_map_points_cam(cur, neighbours, median_depth, cur_model, nb_models, device=0, record_cap=None, **params):
    """dvmh_create_new_map_points_cam: the host entry on a CameraModel per keyframe.  Arguments and result as
    NewPoints.create_new_map_points_cam."""
    keep = []
    cv, k = keyframe_view(cur); keep.append(k)
    n_nb = len(neighbours)
    views = (_KeyFrameView * max(n_nb, 1))()
    models = (CameraModel * max(n_nb, 1))()
    for j, kf in enumerate(neighbours):
        v, k = keyframe_view(kf); keep.append(k)
        views[j] = v
        models[j] = nb_models[j]
    md = np.ascontiguousarray(median_depth, np.float32)
    p = _np_params(cur, **params)
    R = _NpResult(cv.N, n_nb, _np_record_cap(cur, n_nb, record_cap))
    rc = _hcall("dvmh_create_new_map_points_cam", C.c_int32, C.c_int32(device), C.byref(cv), _model_ref(cur_model), C.c_int32(n_nb), C.byref(views), C.byref(models),
                C.c_void_p(md.ctypes.data if md.size else None), C.byref(p), C.byref(R.out))
    check(rc)
    return R.result()


# ---------------------------------------------------------------------------------------------------------------------
# dvm_fuse_targets: the Fuse searches of LocalMapping::SearchInNeighbors against all target keyframes as one chain
class _FtTarget(C.Structure):   # == dvm_ft_target
    _fields_ = [("n", C.c_int32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("Tcw", C.c_float * 7), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("scale_factors", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("log_scale_factor", C.c_float), ("n_levels", C.c_int32)]


class _FtPoints(C.Structure):   # == dvm_ft_points
    _fields_ = [("n", C.c_int32), ("pos", C.c_void_p), ("normal", C.c_void_p), ("min_dist", C.c_void_p), ("max_dist", C.c_void_p),
                ("desc", C.c_void_p), ("valid", C.c_void_p)]


class _FtPointsResident(C.Structure):   # == dvm_ft_points_resident
    _fields_ = [("points", C.c_void_p), ("n", C.c_int32), ("slot", C.c_void_p), ("valid", C.c_void_p)]


class _FtCandidates(C.Structure):   # == dvm_ft_candidates
    _fields_ = [("points", C.c_void_p), ("n_lists", C.c_int32), ("mp_slot", C.c_void_p), ("n", C.c_void_p), ("exclude", C.c_void_p),
                ("n_exclude", C.c_int32)]


HIT_DTYPE = np.dtype([("point", "<i4"), ("idx", "<i4"), ("dist", "<i4")])   # == dvm_ft_hit


class FuseTargets(_Chain):
    """dvm_fuse_targets: set() the target keyframes once (one upload, all grids in one launch), run() point tables against them."""
    FORM_POINTS, FORM_SCW = 0, 1

    def __init__(self, device=0):
        self.n_targets = 0
        super().__init__("dvm_fuse_targets", 2, device)
        vp = C.c_void_p
        self.L.dvm_fuse_targets_set.argtypes = [vp, C.c_int32, vp]
        self.L.dvm_fuse_targets_run.argtypes = [vp, vp, vp, C.c_float, vp, vp]
        self.L.dvm_fuse_targets_set_cam.argtypes = [vp, C.c_int32, vp, vp, vp]
        self.L.dvm_fuse_targets_reserve_hits.argtypes = [vp, C.c_int32]
        self.L.dvm_fuse_targets_run_hits.argtypes = [vp, vp, vp, C.c_float, vp, vp, C.c_int32, vp]
        for f in (self.L.dvm_fuse_targets_set_cam, self.L.dvm_fuse_targets_reserve_hits, self.L.dvm_fuse_targets_run_hits):
            f.restype = C.c_int32

    def reserve(self, max_points, max_targets, max_total_target_keypoints):
        self._reserve(max_points, max_targets, max_total_target_keypoints)

    def last_kernel_ms(self):
        """(grid build of the last set, search of the last run) in milliseconds, with profiling on."""
        return self._last_kernel_ms()

    @staticmethod
    def targets(kfs):
        """Keyframe dicts (kps, desc, Tcw, K, bounds, scale_factors, inv_level_sigma2, log_scale_factor) -> (dvm_ft_target array, keepalive).
        Ow is derived as KeyFrame::SetPose does (Twc's translation)."""
        keep = []
        arr = (_FtTarget * max(len(kfs), 1))()
        for t, kf in enumerate(kfs):
            v, k = keyframe_view(kf)
            keep.append(k)
            s = arr[t]
            s.n, s.kps, s.desc = v.N, v.mvKeysUn, v.mDescriptors
            s.Tcw = v.Tcw
            s.Ow = (C.c_float * 3)(*v.Twc[4:7])
            s.fx, s.fy, s.cx, s.cy = v.fx, v.fy, v.cx, v.cy
            s.min_x, s.max_x, s.min_y, s.max_y = v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY
            s.scale_factors, s.inv_level_sigma2 = v.mvScaleFactors, v.mvInvLevelSigma2
            s.log_scale_factor, s.n_levels = v.mfLogScaleFactor, v.nLevels
        return arr, keep

    def set(self, kfs, models=None, forms=None):
        """models: one CameraModel per target (dvm_fuse_targets_set_cam; under model 1 a keyframe's K is not read and may be absent), forms:
        one of FORM_POINTS / FORM_SCW per target (under FORM_SCW the keyframe's "Tcw" and "Ow" are what sim3_to_se3(Scw) returns; without
        an "Ow" key the centre is derived from Tcw); both None: dvm_fuse_targets_set."""
        arr, keep = self.targets(kfs)
        for t, kf in enumerate(kfs):
            if kf.get("Ow") is not None:
                arr[t].Ow = (C.c_float * 3)(*np.asarray(kf["Ow"], np.float32).reshape(3))
        if models is None and forms is None:
            return self.set_raw(arr, len(kfs))
        m = None
        if models is not None:
            m = (CameraModel * max(len(kfs), 1))()
            for t, x in enumerate(models):
                m[t] = x
        f = None if forms is None else np.ascontiguousarray(forms, np.uint8)
        check(self.L.dvm_fuse_targets_set_cam(self.h, len(kfs), C.addressof(arr), None if m is None else C.addressof(m), _ptr(f)))
        self.n_targets = len(kfs)

    def set_raw(self, arr, n):
        check(self.L.dvm_fuse_targets_set(self.h, int(n), C.addressof(arr)))
        self.n_targets = int(n)

    @staticmethod
    def resident_targets(slots, poses):
        """(dvm_ft_target_resident array) of slots[t] under poses[t]: a 7-float Tcw (the centre is derived as KeyFrame::SetPose does, Twc's
        translation) or a (Tcw, Ow) pair (the Scw form: what sim3_to_se3(Scw) returns)."""
        arr = (_FtTargetResident * max(len(slots), 1))()
        for t, (sl, pose) in enumerate(zip(slots, poses)):
            Tcw, Ow = pose if isinstance(pose, (tuple, list)) and len(pose) == 2 else (pose, None)
            Tcw = np.asarray(Tcw, np.float32).reshape(7)
            Ow = se3_inverse(Tcw)[4:7] if Ow is None else np.asarray(Ow, np.float32).reshape(3)
            arr[t].slot = int(sl); arr[t].Tcw = (C.c_float * 7)(*Tcw); arr[t].Ow = (C.c_float * 3)(*Ow)
        return arr

    def set_resident(self, store, slots, poses, models=None, forms=None):
        """dvm_fuse_targets_set_resident: target t is slot slots[t] of `store` (a KeyframeStore) under poses[t] (resident_targets);
        models / forms as set().  Only the target table travels; run() / run_hits() follow as after set()."""
        assert len(slots) == len(poses)
        arr = self.resident_targets(slots, poses)
        self.set_resident_raw(store, arr, len(slots), models, forms)

    def set_resident_raw(self, store, arr, n, models=None, forms=None):
        m = None
        if models is not None:
            m = (CameraModel * max(n, 1))()
            for t, x in enumerate(models):
                m[t] = x
        f = None if forms is None else np.ascontiguousarray(forms, np.uint8)
        fn = self.L.dvm_fuse_targets_set_resident
        fn.restype = C.c_int32; fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        check(fn(self.h, store.h, int(n), C.addressof(arr), None if m is None else C.addressof(m), _ptr(f)))
        self.n_targets = int(n)

    def last_upload_bytes(self):
        """(set_bytes, run_bytes): the host-to-device bytes queued by the last set (uploaded or resident) and the last run."""
        a, b = C.c_int64(0), C.c_int64(0)
        fn = self.L.dvm_fuse_targets_last_upload_bytes
        fn.restype = C.c_int32; fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        check(fn(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def reserve_hits(self, max_hits):
        check(self.L.dvm_fuse_targets_reserve_hits(self.h, int(max_hits)))

    def run_hits(self, pts, th=3.0, skip=None, hit_cap=None, guard=0):
        """dvm_fuse_targets_run_hits.  Returns (hit_off[T + 1], hits[n_hits] of HIT_DTYPE); hit_cap None: as many as there can be.  A
        DvmError of code -3 carries hit_off and n_hits (the full counts) and, with guard > 0, `tail`: the guard entries behind hits[hit_cap]."""
        P, keep = map_points_view(pts)
        n, T = P.n, self.n_targets
        s = _FtPoints()
        s.n, s.pos, s.normal, s.min_dist, s.max_dist, s.desc = n, P.pos, P.normal, P.min_dist, P.max_dist, P.desc
        va = None if pts.get("valid") is None else np.ascontiguousarray(pts["valid"], np.uint8)
        s.valid = _ptr(va)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(T, n)
        cap = T * n if hit_cap is None else int(hit_cap)
        off = np.full(T + 1, -7, np.int32)
        hits = np.empty(cap + guard + 1, HIT_DTYPE)
        hits.view(np.int32)[3 * cap:] = -7
        nh = C.c_int32(-7)
        rc = self.L.dvm_fuse_targets_run_hits(self.h, C.addressof(s), _ptr(sk), float(th), _ptr(off), _ptr(hits), cap, C.byref(nh))
        try:
            check(rc)
        except DvmError as e:
            e.hit_off, e.n_hits, e.tail = off, nh.value, hits[cap:cap + guard].copy()
            raise
        return off, hits[:nh.value]

    def run(self, pts, th=3.0, skip=None, want_dist=True):
        """pts: dict(pos, normal, min_dist, max_dist, desc[, valid]); skip: [T, n] uint8 or None.  Returns (best_idx[T, n], best_dist[T, n])
        (best_dist None with want_dist = False)."""
        P, keep = map_points_view(pts)
        n, T = P.n, self.n_targets
        s = _FtPoints()
        s.n, s.pos, s.normal, s.min_dist, s.max_dist, s.desc = n, P.pos, P.normal, P.min_dist, P.max_dist, P.desc
        va = None if pts.get("valid") is None else np.ascontiguousarray(pts["valid"], np.uint8)
        s.valid = _ptr(va)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(T, n)
        bi = np.full((T, n), -7, np.int32); bd = np.full((T, n), -7, np.int32) if want_dist else None
        check(self.L.dvm_fuse_targets_run(self.h, C.addressof(s), _ptr(sk), float(th), _ptr(bi), _ptr(bd)))
        return bi, bd

    def _points_resident(self, store, slots, skip, valid):
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n, T = len(slots), self.n_targets
        va = None if valid is None else np.ascontiguousarray(valid, np.uint8).reshape(n)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(T, n)
        s = _FtPointsResident(None if store is None else store.h, n, _ptr(slots), _ptr(va))
        return s, sk, (slots, va)

    def run_resident(self, store, slots, th=3.0, skip=None, valid=None, want_dist=True, out=None):
        """dvm_fuse_targets_run_resident: run() on the records of `store` (a MapStore, or None when every slot is -1) under slots [n]
        (-1: a masked row); a bad record masks its row on the device.  out: (best_idx, best_dist) arrays of the caller's to fill."""
        s, sk, keep = self._points_resident(store, slots, skip, valid)
        n, T = s.n, self.n_targets
        bi, bd = out if out is not None else (np.full((T, n), -7, np.int32), np.full((T, n), -7, np.int32) if want_dist else None)
        fn = self.L.dvm_fuse_targets_run_resident
        fn.restype = C.c_int32; fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        check(fn(self.h, C.addressof(s), _ptr(sk), float(th), _ptr(bi), _ptr(bd)))
        return bi, bd

    def run_hits_resident(self, store, slots, th=3.0, skip=None, valid=None, hit_cap=None, guard=0):
        """dvm_fuse_targets_run_hits_resident; arguments as run_resident, result and DvmError as run_hits."""
        s, sk, keep = self._points_resident(store, slots, skip, valid)
        n, T = s.n, self.n_targets
        cap = T * n if hit_cap is None else int(hit_cap)
        off = np.full(T + 1, -7, np.int32)
        hits = np.empty(cap + guard + 1, HIT_DTYPE)
        hits.view(np.int32)[3 * cap:] = -7
        nh = C.c_int32(-7)
        fn = self.L.dvm_fuse_targets_run_hits_resident
        fn.restype = C.c_int32; fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        rc = fn(self.h, C.addressof(s), _ptr(sk), float(th), _ptr(off), _ptr(hits), cap, C.byref(nh))
        try:
            check(rc)
        except DvmError as e:
            e.hit_off, e.n_hits, e.tail = off, nh.value, hits[cap:cap + guard].copy()
            raise
        return off, hits[:nh.value]

    def reserve_candidates(self, max_entries, map_capacity):
        fn = self.L.dvm_fuse_targets_reserve_candidates
        fn.restype = C.c_int32; fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        check(fn(self.h, int(max_entries), int(map_capacity)))

    def run_hits_candidates(self, store, lists, th=3.0, exclude=None, cand_cap=None, hit_cap=None, guard=0):
        """dvm_fuse_targets_run_hits_candidates: lists = the target keyframes' GetMapPointMatches() as slots of `store`, exclude = the
        current keyframe's.  Returns (cand_slot[n_cand], hit_off[T + 1], hits[n_hits]) with hits["point"] an index into cand_slot.  A
        DvmError of code -3 carries n_cand, hit_off, n_hits and, with guard > 0, `cand_tail`: the guard words behind cand_slot[cand_cap]."""
        lists = [np.ascontiguousarray(a, np.int32).reshape(-1) for a in lists]
        L, T = len(lists), self.n_targets
        total = sum(len(a) for a in lists)
        ptrs = (C.c_void_p * max(L, 1))(*[a.ctypes.data for a in lists])
        lens = np.array([len(a) for a in lists], np.int32)
        ex = None if exclude is None else np.ascontiguousarray(exclude, np.int32).reshape(-1)
        c = _FtCandidates(None if store is None else store.h, L, C.addressof(ptrs), _ptr(lens), _ptr(ex), 0 if ex is None else len(ex))
        ccap = total if cand_cap is None else int(cand_cap)
        cap = T * total if hit_cap is None else int(hit_cap)
        cand = np.full(ccap + guard + 1, -7, np.int32)
        off = np.full(T + 1, -7, np.int32)
        hits = np.empty(cap + 1, HIT_DTYPE)
        nc, nh = C.c_int32(-7), C.c_int32(-7)
        fn = self.L.dvm_fuse_targets_run_hits_candidates
        fn.restype = C.c_int32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        rc = fn(self.h, C.addressof(c), float(th), _ptr(cand), ccap, C.byref(nc), _ptr(off), _ptr(hits), cap, C.byref(nh))
        try:
            check(rc)
        except DvmError as e:
            e.n_cand, e.hit_off, e.n_hits, e.cand_tail = nc.value, off, nh.value, cand[ccap:ccap + guard].copy()
            raise
        return cand[:nc.value], off, hits[:nh.value]


def fuse_targets(kfs, P, in_kf, th, device=0):
    """dvmh_fuse_targets: kfs = keyframe_view() results, P = map_points_view() result, in_kf [T, n] or None.
    Returns (count, best_idx[T, n])."""
    T, n = len(kfs), P[0].n
    views = (_KeyFrameView * max(T, 1))()
    for t, kv in enumerate(kfs):
        views[t] = kv[0]
    bi = np.full((T, n), -7, np.int32)
    ik = None if in_kf is None else np.ascontiguousarray(in_kf, np.uint8).reshape(T, n)
    rc = _hcall("dvmh_fuse_targets", C.c_int32, C.c_int32(device), C.c_int32(T), C.byref(views), C.byref(P[0]), C.c_void_p(_ptr(ik)), C.c_float(th),
                C.c_void_p(_ptr(bi)))
    check(min(rc, 0))
    return rc, bi


def _views_and_models(kfs, models):
    T = len(kfs)
    views = (_KeyFrameView * max(T, 1))()
    for t, kv in enumerate(kfs):
        views[t] = kv[0]
    m = None
    if models is not None:
        m = (CameraModel * max(T, 1))()
        for t, x in enumerate(models):
            m[t] = x
    return views, m


def fuse_targets_cam(kfs, models, P, in_kf, th, device=0):
    """dvmh_fuse_targets_cam: fuse_targets with one CameraModel per keyframe (None: fuse_targets).  Returns (count, best_idx[T, n])."""
    T, n = len(kfs), P[0].n
    views, m = _views_and_models(kfs, models)
    bi = np.full((T, n), -7, np.int32)
    ik = None if in_kf is None else np.ascontiguousarray(in_kf, np.uint8).reshape(T, n)
    rc = _hcall("dvmh_fuse_targets_cam", C.c_int32, C.c_int32(device), C.c_int32(T), C.byref(views), None if m is None else C.byref(m), C.byref(P[0]),
                C.c_void_p(_ptr(ik)), C.c_float(th), C.c_void_p(_ptr(bi)))
    check(min(rc, 0))
    return rc, bi


def fuse_sim3_targets(kfs, Scws, P, th, models=None, hit_cap=None, device=0):
    """dvmh_fuse_sim3_targets: the search part of Fuse(pKF, Scw, vpPoints, th, .) for all keyframes as one chain.  kfs = keyframe_view()
    results (with their mp arrays), Scws [T, 7] Sim3f.  Returns (hit_off[T + 1], hits[n_hits] of HIT_DTYPE); a DvmError of code -3 carries
    hit_off (the full counts)."""
    T, n = len(kfs), P[0].n
    views, m = _views_and_models(kfs, models)
    S = (_Sim3View * max(T, 1))()
    for t in range(T):
        S[t] = _sim3_view(Scws[t])
    cap = T * n if hit_cap is None else int(hit_cap)
    off = np.full(T + 1, -7, np.int32)
    hits = np.empty(cap + 1, HIT_DTYPE)
    rc = _hcall("dvmh_fuse_sim3_targets", C.c_int32, C.c_int32(device), C.c_int32(T), C.byref(views), C.byref(S), None if m is None else C.byref(m),
                C.byref(P[0]), C.c_float(th), C.c_void_p(_ptr(off)), C.c_void_p(_ptr(hits)), C.c_int32(cap))
    try:
        check(min(rc, 0))
    except DvmError as e:
        e.hit_off = off
        raise
    return off, hits[:rc]


def fuse_sim3_apply(KF, P, hits):
    """dvmh_fuse_sim3_apply (host code only): the apply step of Fuse(pKF, Scw, ...) from one keyframe's hits; KF's mp array is updated in
    place.  Returns (nFused, replace)."""
    hits = np.ascontiguousarray(hits, HIT_DTYPE)
    rep = np.zeros(max(P[0].n, 1), np.int32)
    n = _hcall("dvmh_fuse_sim3_apply", C.c_int32, C.byref(KF[0]), C.byref(P[0]), C.c_void_p(_ptr(hits)), C.c_int32(len(hits)), C.c_void_p(rep.ctypes.data))
    if n < 0:
        raise DvmError(n, "dvmh_fuse_sim3_apply: bad argument")
    return n, rep[:P[0].n]


# ---------------------------------------------------------------------------------------------------------------------
# dvm_search_by_bow_targets: the SearchByBoW calls of LoopClosing::DetectCommonRegionsFromBoW against all candidates and covisibles as one chain
# dvm_keyframe_store: keyframes resident on the device, read by FuseTargets.set_resident and NewPoints.create_new_map_points_resident
class _KfsKeyframe(C.Structure):   # == dvm_kfs_keyframe
    _fields_ = [("n", C.c_int32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("fv_n", C.c_int32), ("fv_node", C.c_void_p), ("fv_off", C.c_void_p),
                ("fv_feat", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("log_scale_factor", C.c_float),
                ("n_levels", C.c_int32)]


class _KfsReadback(C.Structure):   # == dvm_kfs_readback
    _fields_ = [("n", C.c_int32), ("fv_n", C.c_int32), ("n_feat", C.c_int32), ("n_levels", C.c_int32), ("n_sorted", C.c_int32), ("n_total", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("log_scale_factor", C.c_float),
                ("generation", C.c_uint32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("fv_node", C.c_void_p), ("fv_off", C.c_void_p),
                ("fv_feat", C.c_void_p), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("inv_level_sigma2", C.c_void_p),
                ("skp", C.c_void_p), ("sidx", C.c_void_p), ("sdesc", C.c_void_p), ("cell_start", C.c_void_p)]


class _KfsDeviceKeyframe(C.Structure):   # == dvm_kfs_device_keyframe
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_n", C.c_void_p), ("n", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("log_scale_factor", C.c_float),
                ("n_levels", C.c_int32)]


class _KfsBowOut(C.Structure):   # == dvm_kfs_bow_out
    _fields_ = [("n", C.c_int32), ("n_bow", C.c_int32), ("n_fv", C.c_int32), ("n_feat", C.c_int32), ("bow_ids", C.c_void_p), ("bow_vals", C.c_void_p),
                ("fv_node", C.c_void_p), ("fv_off", C.c_void_p), ("fv_feat", C.c_void_p)]


def _dev_ptr(v):
    """A torch CUDA tensor, an int device pointer or None -> the pointer (None: NULL)."""
    if v is None:
        return None
    if hasattr(v, "data_ptr"):
        assert v.is_cuda and v.is_contiguous()
        return v.data_ptr()
    return int(v)


class _FtTargetResident(C.Structure):   # == dvm_ft_target_resident
    _fields_ = [("slot", C.c_int32), ("Tcw", C.c_float * 7), ("Ow", C.c_float * 3)]


class _NpKeyFrameResident(C.Structure):   # == dvm_np_keyframe_resident
    _fields_ = [("slot", C.c_int32), ("mp", C.c_void_p), ("Tcw", C.c_float * 7), ("Twc", C.c_float * 7), ("Ow", C.c_float * 3)]


class _NpNeighbourResident(C.Structure):   # == dvm_np_neighbour_resident
    _fields_ = [("kf", _NpKeyFrameResident), ("median_depth", C.c_float), ("ep", C.c_float * 2), ("F12", C.c_float * 9)]


KFS_CELL_START = 64 * 48 + 4       # entries of a slot's cell_start (kCellStartStride)


class KeyframeStore:
    """dvm_keyframe_store: `capacity` slots of up to `slot_keypoints` keypoints in device memory, each holding what a keyframe keeps once
    ComputeBoW has run -- keypoints, descriptors, FeatureVector, level tables, bounds -- and its feature grid.  put() writes keyframes to
    slots (asynchronous; every later chain call that reads the store sees it), remove() empties slots, read() returns one slot (tests).
    Calls on one store are not concurrent; the store outlives the chain handles set on it."""

    def __init__(self, capacity, slot_keypoints, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        vp, i32 = C.c_void_p, C.c_int32
        for name, args in (("create", [i32, i32, i32, vp]), ("capacity", [vp]), ("slot_keypoints", [vp]), ("put", [vp, i32, vp, vp]), ("remove", [vp, i32, vp]),
                           ("debug_read", [vp, i32, vp]), ("put_device", [vp, vp, i32, vp, i32, vp, vp, vp]),
                           ("put_tracked", [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]), ("last_put_bytes", [vp, vp]), ("profile", [vp, i32]),
                           ("last_put_ms", [vp, vp]), ("set_rows", [vp, i32, vp, i32, vp, vp]), ("patch_rows", [vp, i32, vp, i32, vp]),
                           ("debug_read_rows", [vp, i32, i32, vp, i32, vp])):
            f = getattr(self.L, "dvm_keyframe_store_" + name, None)
            if f is None:       # an older library (DVM_HIP_LIB, the measurement tools' baseline): calling the entry raises AttributeError
                continue
            f.restype = i32; f.argtypes = args
        self.L.dvm_keyframe_store_destroy.restype = None; self.L.dvm_keyframe_store_destroy.argtypes = [vp]
        check(self.L.dvm_keyframe_store_create(int(device), int(capacity), int(slot_keypoints), C.byref(self.h)))

    @property
    def capacity(self):
        return self.L.dvm_keyframe_store_capacity(self.h)

    @property
    def slot_keypoints(self):
        return self.L.dvm_keyframe_store_slot_keypoints(self.h)

    @staticmethod
    def records(kfs):
        """Keyframe dicts (kps, desc, fv, K, bounds, scale_factors, level_sigma2, inv_level_sigma2, log_scale_factor; the keys keyframe_view
        takes, a missing one NULL / 0) -> (dvm_kfs_keyframe array, keepalive)."""
        keep = []
        arr = (_KfsKeyframe * max(len(kfs), 1))()
        for t, kf in enumerate(kfs):
            v, k = keyframe_view(kf)
            keep.append(k)
            s = arr[t]
            s.n, s.kps, s.desc = v.N, v.mvKeysUn, v.mDescriptors
            s.fv_n, s.fv_node, s.fv_off, s.fv_feat = v.mFeatVec.n, v.mFeatVec.node, v.mFeatVec.off, v.mFeatVec.feat
            s.fx, s.fy, s.cx, s.cy = v.fx, v.fy, v.cx, v.cy
            s.min_x, s.max_x, s.min_y, s.max_y = v.mnMinX, v.mnMaxX, v.mnMinY, v.mnMaxY
            s.scale_factors, s.level_sigma2, s.inv_level_sigma2 = v.mvScaleFactors, v.mvLevelSigma2, v.mvInvLevelSigma2
            s.log_scale_factor, s.n_levels = v.mfLogScaleFactor, v.nLevels
        return arr, keep

    def put(self, slots, kfs):
        slots = np.ascontiguousarray(slots, np.int32)
        assert slots.ndim == 1 and len(slots) == len(kfs)
        arr, keep = self.records(kfs)
        self.put_raw(slots, arr)

    def put_raw(self, slots, arr):
        check(self.L.dvm_keyframe_store_put(self.h, len(slots), _p(slots), C.addressof(arr)))

    @staticmethod
    def device_records(kfs):
        """Keyframe dicts -> (dvm_kfs_device_keyframe array, keepalive).  kps / desc: torch CUDA tensors or int device pointers (missing:
        NULL); n: the device count, a tensor or an int device pointer, or None / missing; count: the host count (without n) or the
        arrays' capacity (with n) -- missing: the length of a kps tensor.  K, bounds, scale_factors, level_sigma2, inv_level_sigma2,
        log_scale_factor, n_levels (default: the scale table's length): as keyframe_view; a missing table is NULL."""
        keep = []
        arr = (_KfsDeviceKeyframe * max(len(kfs), 1))()
        for t, kf in enumerate(kfs):
            s = arr[t]
            kps = kf.get("kps")
            keep.append([kps, kf.get("desc"), kf.get("n")])
            s.d_kps, s.d_desc, s.d_n = _dev_ptr(kps), _dev_ptr(kf.get("desc")), _dev_ptr(kf.get("n"))
            if kf.get("count") is not None:
                s.n = int(kf["count"])
            else:
                s.n = kps.numel() * kps.element_size() // KP_DTYPE.itemsize if hasattr(kps, "numel") else 0
            s.fx, s.fy, s.cx, s.cy = (float(x) for x in kf.get("K", (0, 0, 0, 0)))
            s.min_x, s.max_x, s.min_y, s.max_y = (float(x) for x in kf["bounds"])
            nl = 0
            for key in ("scale_factors", "level_sigma2", "inv_level_sigma2"):
                if kf.get(key) is not None:
                    a = np.ascontiguousarray(kf[key], np.float32); keep.append(a); setattr(s, key, a.ctypes.data); nl = len(a)
            s.n_levels = int(kf.get("n_levels", nl))
            s.log_scale_factor = float(kf.get("log_scale_factor", 0.0))
        return arr, keep

    def _bow_outs(self, n):
        K = self.slot_keypoints
        outs = (_KfsBowOut * max(n, 1))()
        bufs = []
        for k in range(n):
            b = dict(bow_ids=np.zeros(K, np.int32), bow_vals=np.zeros(K, np.float64), fv_node=np.zeros(K, np.int32), fv_off=np.zeros(K + 1, np.int32),
                     fv_feat=np.zeros(K, np.int32))
            for name, a in b.items():
                setattr(outs[k], name, a.ctypes.data)
            bufs.append(b)
        return outs, bufs

    @staticmethod
    def _bow_results(outs, bufs):
        return [dict(n=o.n, bow_ids=b["bow_ids"][:o.n_bow].copy(), bow_vals=b["bow_vals"][:o.n_bow].copy(), fv_nodes=b["fv_node"][:o.n_fv].copy(),
                     fv_off=b["fv_off"][:o.n_fv + 1].copy(), fv_feat=b["fv_feat"][:o.n_feat].copy()) for o, b in zip(outs, bufs)]

    def put_device(self, voc, slots, kfs, levelsup=4, stream=None):
        """dvm_keyframe_store_put_device: keyframes whose arrays are in device memory (device_records) go to `slots`; KeyFrame::ComputeBoW
        runs on the device.  voc: a Vocabulary; stream: the stream that produced the arrays (an int handle; None: the null stream).
        One synchronisation.  Returns a list of dict(n, bow_ids, bow_vals, fv_nodes, fv_off, fv_feat) as vocab_transform_host."""
        slots = np.ascontiguousarray(slots, np.int32)
        assert slots.ndim == 1 and len(slots) == len(kfs)
        arr, keep = self.device_records(kfs)
        outs, bufs = self._bow_outs(len(kfs))
        check(self.L.dvm_keyframe_store_put_device(self.h, voc.h, int(levelsup), stream, len(slots), _p(slots), C.addressof(arr), C.addressof(outs)))
        return self._bow_results(outs[:len(kfs)], bufs)

    def put_tracked(self, tracker, ext, voc, frames, slots, tables, levelsup=4):
        """dvm_keyframe_store_put_tracked: frames `frames` of the last finish of `tracker` (a Tracker or a TrackerBatch on extractor `ext`)
        go to `slots`.  tables: per keyframe dict(K, bounds, scale_factors, level_sigma2, inv_level_sigma2, log_scale_factor).
        Returns what put_device returns."""
        frames = np.ascontiguousarray(frames, np.int32); slots = np.ascontiguousarray(slots, np.int32)
        assert frames.ndim == 1 and slots.ndim == 1 and len(frames) == len(slots) == len(tables)
        arr, keep = self.device_records([dict(t, kps=None, desc=None, n=None, count=0) for t in tables])
        outs, bufs = self._bow_outs(len(tables))
        check(self.L.dvm_keyframe_store_put_tracked(self.h, tracker.t, ext.h, voc.h, int(levelsup), len(slots), _p(frames), _p(slots), C.addressof(arr),
                                                    C.addressof(outs)))
        return self._bow_results(outs[:len(tables)], bufs)

    def last_put_bytes(self):
        """Host-to-device bytes of the last put or put_device that reached the device."""
        b = C.c_int64(0)
        check(self.L.dvm_keyframe_store_last_put_bytes(self.h, C.byref(b)))
        return b.value

    def profile(self, on=True):
        check(self.L.dvm_keyframe_store_profile(self.h, int(on)))

    def last_put_ms(self):
        """(check, transform, bow, put) milliseconds of the last put_device that ran with profiling on (its first round)."""
        ms = (C.c_float * 4)()
        check(self.L.dvm_keyframe_store_last_put_ms(self.h, ms))
        return tuple(ms)

    def remove(self, slots):
        slots = np.ascontiguousarray(slots, np.int32)
        check(self.L.dvm_keyframe_store_remove(self.h, len(slots), _p(slots)))

    def read(self, slot):
        """One slot back (synchronous): dict(n, fv_n, n_feat, n_levels, n_sorted, n_total, generation, K, bounds, log_scale_factor, kps,
        desc, fv_nodes, fv_off, fv_feat, scale_factors, level_sigma2, inv_level_sigma2, skp[n_sorted, 4], sidx, sdesc, cell_start)."""
        K = self.slot_keypoints
        a = dict(kps=np.zeros(K, KP_DTYPE), desc=np.zeros((K, 32), np.uint8), fv_node=np.zeros(K, np.int32), fv_off=np.zeros(K + 1, np.int32),
                 fv_feat=np.zeros(K, np.int32), scale_factors=np.zeros(64, np.float32), level_sigma2=np.zeros(64, np.float32),
                 inv_level_sigma2=np.zeros(64, np.float32), skp=np.zeros((K, 4), np.float32), sidx=np.zeros(K, np.int32),
                 sdesc=np.zeros((K, 32), np.uint8), cell_start=np.zeros(KFS_CELL_START, np.int32))
        r = _KfsReadback()
        for k, v in a.items():
            setattr(r, k, v.ctypes.data)
        check(self.L.dvm_keyframe_store_debug_read(self.h, int(slot), C.addressof(r)))
        n, ns, nl = r.n, r.n_sorted, r.n_levels
        return dict(n=n, fv_n=r.fv_n, n_feat=r.n_feat, n_levels=nl, n_sorted=ns, n_total=r.n_total, generation=r.generation,
                    K=np.array([r.fx, r.fy, r.cx, r.cy], np.float32), bounds=np.array([r.min_x, r.max_x, r.min_y, r.max_y], np.float32),
                    log_scale_factor=r.log_scale_factor, kps=a["kps"][:n].copy(), desc=a["desc"][:n].copy(), fv_nodes=a["fv_node"][:r.fv_n].copy(),
                    fv_off=a["fv_off"][:r.fv_n + 1 if r.fv_n else 0].copy(), fv_feat=a["fv_feat"][:r.n_feat].copy(),
                    scale_factors=a["scale_factors"][:nl].copy(), level_sigma2=a["level_sigma2"][:nl].copy(),
                    inv_level_sigma2=a["inv_level_sigma2"][:nl].copy(), skp=a["skp"][:ns].copy(), sidx=a["sidx"][:ns].copy(),
                    sdesc=a["sdesc"][:ns].copy(), cell_start=a["cell_start"])

    def set_rows(self, which, points, slots, rows):
        """dvm_keyframe_store_set_rows: rows[k] (int32, as long as the slot's n; None: a NULL row) becomes the row of kind `which`
        (KFS_ROW_MATCHES / KFS_ROW_OBSERVED) of slot slots[k]; its values are slots of the MapStore `points` or -1.  Asynchronous."""
        slots = np.ascontiguousarray(slots, np.int32)
        assert slots.ndim == 1 and len(slots) == len(rows)
        keep = [None if r is None else np.ascontiguousarray(r, np.int32) for r in rows]
        ptrs = (C.c_void_p * max(len(keep), 1))(*[None if r is None else r.ctypes.data for r in keep])
        check(self.L.dvm_keyframe_store_set_rows(self.h, int(which), None if points is None else points.h, len(slots), _p(slots), C.addressof(ptrs)))

    def patch_rows(self, which, points, edits):
        """dvm_keyframe_store_patch_rows: edits = KFS_ROW_EDIT_DTYPE records or (slot, kp, value) triples, applied in order."""
        e = np.asarray(edits)
        if e.dtype != KFS_ROW_EDIT_DTYPE:
            e = np.ascontiguousarray(e, np.int32).reshape(-1, 3).view(KFS_ROW_EDIT_DTYPE).reshape(-1)
        e = np.ascontiguousarray(e)
        check(self.L.dvm_keyframe_store_patch_rows(self.h, int(which), None if points is None else points.h, len(e), _p(e)))

    def read_rows(self, which, slot):
        """One row back (synchronous, tests): int32 [n], empty for a row that is not set."""
        out = np.full(self.slot_keypoints, -7, np.int32)
        n = C.c_int32(-7)
        check(self.L.dvm_keyframe_store_debug_read_rows(self.h, int(which), int(slot), _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.dvm_keyframe_store_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close


# ---- Tracking::UpdateLocalMap on the resident stores (dvm_update_local_map, include/dvmslam_hip.h)
KFS_ROW_MATCHES, KFS_ROW_OBSERVED = 0, 1
KFS_ROW_EDIT_DTYPE = np.dtype([("slot", "<i4"), ("kp", "<i4"), ("value", "<i4")])      # == dvm_kfs_row_edit


class _UlmKeyframesIn(C.Structure):   # == dvm_ulm_keyframes_in
    _fields_ = [("kfs", C.c_void_p), ("points", C.c_void_p), ("n", C.c_int32), ("mp_slot", C.c_void_p)]


class _UlmKeyframesOut(C.Structure):   # == dvm_ulm_keyframes_out
    _fields_ = [("votes", C.c_void_p), ("frame_bad", C.c_void_p)]


class _UlmPointsIn(C.Structure):   # == dvm_ulm_points_in
    _fields_ = [("kfs", C.c_void_p), ("points", C.c_void_p), ("n_kfs", C.c_int32), ("kf_slot", C.c_void_p), ("n", C.c_int32), ("mp_slot", C.c_void_p)]


class _UlmPointsOut(C.Structure):   # == dvm_ulm_points_out
    _fields_ = [("local_slot", C.c_void_p), ("local_cap", C.c_int32), ("n_local", C.c_int32), ("frame_mp", C.c_void_p), ("n_outside", C.c_int32)]


class UpdateLocalMap:
    """dvm_update_local_map: the vote loop of UpdateLocalKeyFrames and UpdateLocalPoints for the frames of one tick, read from the rows a
    KeyframeStore keeps (set_rows / patch_rows) and the records of a MapStore.  A frame is a dict; every call is one upload, one chain of
    launches and one synchronisation."""

    GUARD = 64       # guard words behind every output array (tests look at them)

    def __init__(self, device=0):
        self.L = lib()
        vp, i32 = C.c_void_p, C.c_int32
        _declare(self.L, {"dvm_update_local_map_create": [i32, vp], "dvm_update_local_map_reserve": [vp, i32, i32, i32, i32, i32, i32],
                          "dvm_update_local_map_keyframes": [vp, i32, vp, vp], "dvm_update_local_map_points": [vp, i32, vp, vp],
                          "dvm_update_local_map_last_bytes": [vp, vp, vp], "dvm_update_local_map_profile": [vp, i32],
                          "dvm_update_local_map_last_ms": [vp, vp]})
        self.L.dvm_update_local_map_destroy.restype = None; self.L.dvm_update_local_map_destroy.argtypes = [vp]
        self.h = vp()
        check(self.L.dvm_update_local_map_create(int(device), C.byref(self.h)))

    def reserve(self, max_frames, max_frame_keypoints, max_local_keyframes, map_capacity, kf_capacity, slot_keypoints):
        check(self.L.dvm_update_local_map_reserve(self.h, int(max_frames), int(max_frame_keypoints), int(max_local_keyframes), int(map_capacity),
                                                  int(kf_capacity), int(slot_keypoints)))

    def keyframes(self, frames):
        """frames: dict(kfs=KeyframeStore, points=MapStore, mp_slot=int32 [n]) per frame.  Returns per frame dict(votes [capacity of kfs],
        frame_bad [n] uint8); the arrays carry GUARD untouched entries behind them under votes_guarded / frame_bad_guarded."""
        B, G = len(frames), self.GUARD
        ins = (_UlmKeyframesIn * max(B, 1))(); outs = (_UlmKeyframesOut * max(B, 1))()
        keep, res = [], []
        for b, f in enumerate(frames):
            mp = np.ascontiguousarray(f["mp_slot"], np.int32)
            votes = np.full(f["kfs"].capacity + G, -7, np.int32); bad = np.full(len(mp) + G, 7, np.uint8)
            keep.append(mp)
            ins[b].kfs, ins[b].points, ins[b].n, ins[b].mp_slot = f["kfs"].h, f["points"].h, len(mp), mp.ctypes.data
            outs[b].votes, outs[b].frame_bad = votes.ctypes.data, bad.ctypes.data
            res.append(dict(votes=votes[:len(votes) - G], frame_bad=bad[:len(mp)], votes_guarded=votes, frame_bad_guarded=bad))
        check(self.L.dvm_update_local_map_keyframes(self.h, B, C.addressof(ins), C.addressof(outs)))
        return res

    def points(self, frames, local_cap=None, raise_capacity=True):
        """frames: dict(kfs, points, kf_slot=int32 [n_kfs], mp_slot=int32 [n]) per frame; local_cap: one value or one per frame (default:
        the map store's capacity).  Returns per frame dict(local_slot [min(n_local, local_cap)], n_local, frame_mp [n], n_outside, and
        the guarded arrays).  With raise_capacity=False a DVM_ERR_CAPACITY call returns its (complete) results with capacity=True."""
        B, G = len(frames), self.GUARD
        ins = (_UlmPointsIn * max(B, 1))(); outs = (_UlmPointsOut * max(B, 1))()
        caps = _per_frame(local_cap, B) if local_cap is not None else [f["points"].capacity for f in frames]
        keep, arrs = [], []
        for b, f in enumerate(frames):
            mp = np.ascontiguousarray(f["mp_slot"], np.int32); kf = np.ascontiguousarray(f["kf_slot"], np.int32)
            loc = np.full(int(caps[b]) + G, -7, np.int32); fmp = np.full(len(mp) + G, -7, np.int32)
            keep.append((mp, kf)); arrs.append((loc, fmp))
            i, o = ins[b], outs[b]
            i.kfs, i.points, i.n_kfs, i.kf_slot, i.n, i.mp_slot = f["kfs"].h, f["points"].h, len(kf), kf.ctypes.data, len(mp), mp.ctypes.data
            o.local_slot, o.local_cap, o.n_local, o.frame_mp, o.n_outside = loc.ctypes.data, int(caps[b]), -7, fmp.ctypes.data, -7
        rc = self.L.dvm_update_local_map_points(self.h, B, C.addressof(ins), C.addressof(outs))
        if rc != -3 or raise_capacity or outs[0].n_local == -7:   # (-3: DVM_ERR_CAPACITY; n_local untouched: refused before it ran)
            check(rc)
        res = []
        for b in range(B):
            loc, fmp = arrs[b]
            o = outs[b]
            res.append(dict(local_slot=loc[:min(o.n_local, int(caps[b]))], n_local=o.n_local, frame_mp=fmp[:len(fmp) - G], n_outside=o.n_outside,
                            local_guarded=loc, frame_mp_guarded=fmp, capacity=rc == -3))
        return res

    def last_bytes(self):
        """(host to device, device to host) of the last call."""
        up, down = C.c_int64(0), C.c_int64(0)
        check(self.L.dvm_update_local_map_last_bytes(self.h, C.byref(up), C.byref(down)))
        return up.value, down.value

    def profile(self, enable=True):
        check(self.L.dvm_update_local_map_profile(self.h, int(bool(enable))))

    def last_ms(self):
        ms = C.c_float(0)
        check(self.L.dvm_update_local_map_last_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.dvm_update_local_map_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close


class _BtKeyFrame(C.Structure):   # == dvm_bt_keyframe
    _fields_ = [("n", C.c_int32), ("fv_n", C.c_int32), ("kps", C.c_void_p), ("desc", C.c_void_p), ("mp", C.c_void_p), ("bad", C.c_void_p),
                ("fv_node", C.c_void_p), ("fv_off", C.c_void_p), ("fv_feat", C.c_void_p)]


class KfResident(C.Structure):   # == dvm_kf_resident
    _fields_ = [("slot", C.c_int32), ("points", C.c_void_p), ("mp_slot", C.c_void_p)]


def _kf_resident(kf, s, keep):
    """(slot, MapStore or None, mp_slots or None) -> dvm_kf_resident s; the slot list is kept alive in keep."""
    slot, store, mp = kf
    a = None if mp is None else np.ascontiguousarray(mp, np.int32)
    keep.append((store, a))
    s.slot = int(slot)
    s.points = None if store is None else store.h
    s.mp_slot = None if a is None else a.ctypes.data


class BowTargets(_Chain):
    """dvm_bow_targets: SearchByBoW(cur, target) (ORBmatcher.cc:709-834) for all target keyframes behind one upload and one synchronisation."""

    def __init__(self, device=0):
        super().__init__("dvm_bow_targets", 2, device)
        vp = C.c_void_p
        self.L.dvm_search_by_bow_targets.argtypes = [vp, vp, C.c_int32, vp, C.c_float, C.c_int32, vp, vp]
        _declare(self.L, {"dvm_search_by_bow_targets_resident": [vp, vp, vp, C.c_int32, vp, C.c_float, C.c_int32, vp, vp],
                          "dvm_bow_targets_last_upload_bytes": [vp, vp], "dvm_bow_targets_last_prologue_ms": [vp, vp]})

    def reserve(self, max_cur_keypoints, max_targets, max_total_target_keypoints):
        self._reserve(max_cur_keypoints, max_targets, max_total_target_keypoints)

    def last_kernel_ms(self):
        """(search, settle) milliseconds of the last call that ran with profiling on."""
        return self._last_kernel_ms()

    @staticmethod
    def _keyframe(kf, s, keep):
        """dict(kps, desc, mp[, bad], fv) -> dvm_bt_keyframe; a key that is missing or None is a NULL array."""
        kps = np.ascontiguousarray(kf["kps"], KP_DTYPE)
        arrs = [kps, None if kf.get("desc") is None else np.ascontiguousarray(kf["desc"], np.uint8),
                None if kf.get("mp") is None else np.ascontiguousarray(kf["mp"], np.int32),
                None if kf.get("bad") is None else np.ascontiguousarray(kf["bad"], np.uint8)]
        fv = kf.get("fv") or {}
        arrs += [None if fv.get(k) is None else np.ascontiguousarray(fv[k], np.int32) for k in ("fv_nodes", "fv_off", "fv_feat")]
        keep.append(arrs)
        s.n = int(kf.get("n", len(kps)))
        s.fv_n = 0 if arrs[4] is None else len(arrs[4])
        s.kps, s.desc, s.mp, s.bad, s.fv_node, s.fv_off, s.fv_feat = (None if a is None else a.ctypes.data for a in arrs)

    def prepare(self, cur, targets, nnratio=0.9, check_ori=True):
        """The argument structs of a call built once: returns run() -> (match_idx2[T, n], nmatches[T]), for a caller that repeats the call
        on the same keyframes (a timing loop).  The arrays are read in place at run()."""
        keep = []
        c = _BtKeyFrame()
        self._keyframe(cur, c, keep)
        T = len(targets)
        arr = (_BtKeyFrame * max(T, 1))()
        for t, kf in enumerate(targets):
            self._keyframe(kf, arr[t], keep)
        n1 = max(int(c.n), 0)
        idx = np.full((T, n1), -7, np.int32); nm = np.full(T, -7, np.int32)

        def run():
            keep  # noqa: B018 (the arrays live as long as the closure)
            check(self.L.dvm_search_by_bow_targets(self.h, C.addressof(c), T, C.addressof(arr), float(nnratio), int(check_ori),
                                                   idx.ctypes.data, nm.ctypes.data))
            return idx, nm
        return run

    def search(self, cur, targets, nnratio=0.9, check_ori=True):
        """cur / targets: keyframe dicts (kps, desc, mp[, bad], fv).  Returns (match_idx2[T, n], nmatches[T])."""
        return self.prepare(cur, targets, nnratio, check_ori)()


    def prepare_resident(self, store, cur, targets, nnratio=0.9, check_ori=True):
        """prepare() for search_resident: the slot lists are read in place at run()."""
        keep = []
        c = KfResident()
        _kf_resident(cur, c, keep)
        T = len(targets)
        arr = (KfResident * max(T, 1))()
        for t, kf in enumerate(targets):
            _kf_resident(kf, arr[t], keep)
        n1 = 0 if keep[0][1] is None else len(keep[0][1])
        idx = np.full((T, n1), -7, np.int32); nm = np.full(T, -7, np.int32)

        def run():
            keep  # noqa: B018 (the arrays live as long as the closure)
            check(self.L.dvm_search_by_bow_targets_resident(self.h, store.h, C.addressof(c), T, C.addressof(arr), float(nnratio), int(check_ori),
                                                            idx.ctypes.data, nm.ctypes.data))
            return idx, nm
        return run

    def search_resident(self, store, cur, targets, nnratio=0.9, check_ori=True):
        """dvm_search_by_bow_targets_resident.  store: the KeyframeStore; cur / targets: (slot, MapStore or None, mp_slots) -- the keyframe's
        slot, the map its points live in and GetMapPointMatches() as that map's slots (-1 = none; as long as the slot's keyframe).
        Returns what search() returns."""
        return self.prepare_resident(store, cur, targets, nnratio, check_ori)()

    def last_upload_bytes(self):
        """dvm_bow_targets_last_upload_bytes: host-to-device bytes of the last call that reached the device, either form."""
        b = C.c_int64(0)
        check(self.L.dvm_bow_targets_last_upload_bytes(self.h, C.byref(b)))
        return b.value

    def last_prologue_ms(self):
        """The prologue kernel's milliseconds of the last resident call that ran with profiling on."""
        ms = C.c_float(0)
        check(self.L.dvm_bow_targets_last_prologue_ms(self.h, C.byref(ms)))
        return ms.value


def search_by_bow_targets(KF1, kfs, nnratio=0.9, check_ori=True, device=0, want_idx2=True):
    """dvmh_search_by_bow_targets: KF1 / kfs = keyframe_view() results.  Returns (sum of nmatches, matches12[T, N] map-point ids,
    idx2[T, N] or None, nmatches[T])."""
    T, n = len(kfs), KF1[0].N
    views = (_KeyFrameView * max(T, 1))()
    for t, kv in enumerate(kfs):
        views[t] = kv[0]
    m12 = np.full((T, n), -7, np.int32); idx2 = np.full((T, n), -7, np.int32) if want_idx2 else None; nm = np.full(T, -7, np.int32)
    rc = _hcall("dvmh_search_by_bow_targets", C.c_int32, C.c_int32(device), C.byref(KF1[0]), C.c_int32(T), C.byref(views), C.c_float(nnratio),
                C.c_int32(int(check_ori)), C.c_void_p(m12.ctypes.data), C.c_void_p(None if idx2 is None else idx2.ctypes.data), C.c_void_p(nm.ctypes.data))
    check(min(rc, 0))
    return rc, m12, idx2, nm
