"""Python mirror of the reference detector interface over the C ABI.

``GpuDetector`` follows frc971::apriltag::GpuDetector
(src/apriltags_cuda/include/apriltags_cuda/apriltag_gpu.h:77-359): construct
once per camera with width, height and calibration, call ``detect(frame)``
per frame, read ``detections()``; the debug copy-outs
(apriltag_gpu.h:98-183) are the ``copy_*`` methods.  Everything runs in
``libat_hip.so`` (HIP kernels for gfx950); there is no CPU fallback: if the
library or a GPU is missing the constructor raises.
"""
import ctypes as C
import math
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AT_HIP_LIB overrides the library (A/B timing of build variants, tools/ab.sh)
LIB_PATH = os.environ.get("AT_HIP_LIB") or os.path.join(_HERE, "libat_hip.so")

AT_FMT_YUYV, AT_FMT_BGR8, AT_FMT_GRAY8 = 0, 1, 2
(AT_STAGE_GRAY, AT_STAGE_DECIMATED, AT_STAGE_THRESHOLD, AT_STAGE_LABELS, AT_STAGE_SIZES,
 AT_STAGE_NUM_POINTS, AT_STAGE_NUM_PAIRS, AT_STAGE_QUADS, AT_STAGE_POINTS, AT_STAGE_BLOB_POINTS,
 AT_STAGE_NUM_PAIR_ENTRIES, AT_STAGE_PROBE) = range(12)
AT_E_INVALID, AT_E_CAPACITY, AT_E_UNSUPPORTED = -1, -3, -6

# Symbols declared in include/at_api.h (checked by tests/test_abi.py).
EXPORTS = [
    "at_config_default", "at_create", "at_detect", "at_detect_batch", "at_detect_device",
    "at_enqueue_device", "at_collect", "at_frame_status", "at_debug_copy", "at_destroy",
    "at_strerror", "at_family_num_known", "at_family_entry", "at_abi_version",
    "at_set_profiling", "at_stage_times", "at_stage_name", "at_poses", "at_tag_detections",
    "at_set_kernel_timer", "at_kernel_time", "at_batch_stats", "at_stream_wait",
    "at_gp_enable", "at_gp_tensor", "at_gp_copy", "at_gp_preprocess_device", "at_set_debug_taps",
    "at_draw_outlines_device", "at_detections", "at_max_detections", "at_annotate_staged", "at_enqueue_host",
    "at_kernel_span", "at_host_alloc", "at_host_free",
    "at_enqueue_mjpg", "at_detect_mjpg", "at_detect_mjpg_batch", "at_mjpg_set_threads", "at_mjpg_stats",
    "at_mjpg_decode_gray_host", "at_mjpg_stream_mode_host",
    "at_mjpg_set_color", "at_mjpg_bgr", "at_mjpg_copy_bgr", "at_mjpg_decode_bgr_host",
    "at_encode_jpeg_device", "at_annotate_jpeg", "at_jpeg_max_bytes", "at_jpeg_stats", "at_jpeg_encode_host",
    "at_gp_parse_host", "at_gp_parse_device", "at_gp_draw_boxes_device", "at_gp_parse_stats",
    "at_gp_annotate_staged", "at_gp_annotate_jpeg", "at_gp_copy_raw",
    "at_mjpg_set_device_entropy", "at_mjpg_set_subseq", "at_mjpg_entropy_host", "at_mjpg_dense_host",
    "at_preview_size", "at_preview_bgr", "at_preview_jpeg", "at_preview_jpeg_device", "at_preview_host",
    "at_preview_jpeg_host", "at_preview_stats",
    "at_set_field_layout", "at_field_poses", "at_field_pose_host", "at_robot_in_field", "at_field_stats",
    "at_rig_create", "at_rig_solve", "at_rig_stats", "at_rig_destroy", "at_rig_pose_host",
    "at_rig_solve_robust", "at_rig_pose_robust_host", "at_rig_robust_stats",
    "at_rigcal_create", "at_rigcal_add", "at_rigcal_count", "at_rigcal_clear", "at_rigcal_solve",
    "at_rigcal_solve_host", "at_rigcal_instants", "at_rigcal_set_profiling", "at_rigcal_stats", "at_rigcal_destroy",
    "at_rigtrack_create", "at_rigtrack_push", "at_rigtrack_count", "at_rigtrack_clear", "at_rigtrack_solve",
    "at_rigtrack_solve_host", "at_rigtrack_instants", "at_rigtrack_set_profiling", "at_rigtrack_stats",
    "at_rigtrack_destroy",
    "at_camcal_create", "at_camcal_add", "at_camcal_count", "at_camcal_clear", "at_camcal_solve",
    "at_camcal_solve_host", "at_camcal_views", "at_camcal_set_profiling", "at_camcal_stats", "at_camcal_destroy",
    "at_fieldmap_create", "at_fieldmap_add", "at_fieldmap_count", "at_fieldmap_clear", "at_fieldmap_solve",
    "at_fieldmap_solve_host", "at_fieldmap_tags", "at_fieldmap_views", "at_fieldmap_set_profiling",
    "at_fieldmap_stats", "at_fieldmap_destroy",
    "at_set_undistort", "at_ideal_detections", "at_ideal_detections_host", "at_undistort_points",
    "at_undistort_points_host", "at_undistort_stats",
]
AT_RIGCAL_MAX_INSTANTS = 4096
AT_RIGTRACK_MAX_WINDOW = 64
AT_CAMCAL_MAX_VIEWS = 4096
AT_FIELDMAP_MAX_TAGS = 32
AT_FIELDMAP_MAX_VIEWS = 4096
# at_camcal_config.free_mask bits, in at_camera's order
CAMCAL_PARAMS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
(AT_CAMCAL_FX, AT_CAMCAL_FY, AT_CAMCAL_CX, AT_CAMCAL_CY, AT_CAMCAL_K1, AT_CAMCAL_K2, AT_CAMCAL_P1, AT_CAMCAL_P2,
 AT_CAMCAL_K3) = (1 << i for i in range(9))
AT_CAMCAL_PINHOLE = AT_CAMCAL_FX | AT_CAMCAL_FY | AT_CAMCAL_CX | AT_CAMCAL_CY
AT_CAMCAL_ALL = 511
AT_FIELD_MAX_TAGS = 16
AT_RIG_MAX_CAMS = 8
AT_GP_MAX_CANDIDATES = 4096
# at_gp_box as a numpy record (the bit-exact view of what the library wrote)
GP_BOX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("conf", "<f4"), ("cls", "<i4")])
JPEG_SAMPLINGS = {"4:2:0": 0, "4:2:2": 1, "4:4:4": 2}  # AT_JPEG_420 / 422 / 444

TAG_SIZE = 0.1651  # metres, apriltags_cuda_detector.hpp:39


class AtConfig(C.Structure):
    _fields_ = [
        ("width", C.c_int), ("height", C.c_int), ("family", C.c_char_p),
        ("quad_decimate", C.c_float), ("refine_edges", C.c_int), ("decode_sharpening", C.c_double),
        ("min_white_black_diff", C.c_int), ("min_cluster_pixels", C.c_int), ("max_nmaxima", C.c_int),
        ("max_line_fit_mse", C.c_float), ("cos_critical_rad", C.c_double),
        ("device", C.c_int), ("max_batch", C.c_int), ("tag_size", C.c_double),
    ]


class AtCamera(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")]


class AtDetection(C.Structure):
    _fields_ = [
        ("id", C.c_int32), ("hamming", C.c_int32), ("decision_margin", C.c_float),
        ("H", C.c_double * 9), ("c", C.c_double * 2), ("p", (C.c_double * 2) * 4),
    ]


class AtPose(C.Structure):
    _fields_ = [("id", C.c_int32), ("R", C.c_double * 9), ("t", C.c_double * 3), ("err", C.c_double)]


class AtTagDetection(C.Structure):
    _fields_ = [("id", C.c_int32), ("camera", C.c_double * 3), ("robot", C.c_double * 3),
                ("distance", C.c_double), ("err", C.c_double)]


class AtFieldTag(C.Structure):
    _fields_ = [("id", C.c_int32), ("R", C.c_double * 9), ("t", C.c_double * 3)]


class AtFieldPose(C.Structure):
    _fields_ = [("n_tags", C.c_int32), ("ids", C.c_int32 * AT_FIELD_MAX_TAGS), ("R", C.c_double * 9),
                ("t", C.c_double * 3), ("rms_px", C.c_double), ("steps_taken", C.c_int32)]


class AtRigExtrinsics(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3)]


class AtRigPose(C.Structure):
    _fields_ = [("n_tags", C.c_int32), ("n_cams_used", C.c_int32), ("tags_per_cam", C.c_int32 * AT_RIG_MAX_CAMS),
                ("ids", (C.c_int32 * AT_FIELD_MAX_TAGS) * AT_RIG_MAX_CAMS), ("R", C.c_double * 9),
                ("t", C.c_double * 3), ("cov", C.c_double * 36), ("rms_px", C.c_double), ("cov_valid", C.c_int32),
                ("steps_taken", C.c_int32), ("rejected", C.c_int32), ("dropped", C.c_int32)]


class AtRigHostCam(C.Structure):
    _fields_ = [("dets", C.POINTER(AtDetection)), ("poses", C.POINTER(AtPose)), ("n", C.c_int32),
                ("cam", C.POINTER(AtCamera)), ("extr", AtRigExtrinsics)]


class AtRigRobustConfig(C.Structure):
    _fields_ = [("huber_px", C.c_double), ("reject_px", C.c_double), ("max_rounds", C.c_int32),
                ("min_keep", C.c_int32)]


class AtRigRobustInfo(C.Structure):
    _fields_ = [("n_kept", C.c_int32), ("n_rejected", C.c_int32), ("rounds", C.c_int32), ("starved", C.c_int32),
                ("rejected_mask", C.c_uint32 * AT_RIG_MAX_CAMS),
                ("tag_rms_px", (C.c_double * AT_FIELD_MAX_TAGS) * AT_RIG_MAX_CAMS), ("huber_cost", C.c_double),
                ("n_downweighted", C.c_int32), ("pad", C.c_int32)]


class AtRigcalCamera(C.Structure):
    _fields_ = [("cam", AtCamera), ("extr", AtRigExtrinsics), ("free_rot", C.c_int32), ("free_trans", C.c_int32)]


class AtRigcalFrame(C.Structure):
    _fields_ = [("dets", C.POINTER(AtDetection)), ("poses", C.POINTER(AtPose)), ("n", C.c_int32)]


class AtRigcalCameraResult(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("cov", C.c_double * 36)]


class AtRigcalResult(C.Structure):
    _fields_ = [("rms_before", C.c_double), ("rms_after", C.c_double), ("instants_used", C.c_int32),
                ("instants_skipped", C.c_int32), ("accepted", C.c_int32), ("rejected", C.c_int32),
                ("cov_valid", C.c_int32), ("n_cams", C.c_int32), ("cams", AtRigcalCameraResult * AT_RIG_MAX_CAMS)]


class AtRigcalInstant(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("rms_px", C.c_double), ("n_tags", C.c_int32),
                ("used", C.c_int32)]


class AtRigtrackCamera(C.Structure):
    _fields_ = [("cam", AtCamera), ("extr", AtRigExtrinsics)]


class AtRigtrackOdom(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("sigma_rot", C.c_double), ("sigma_trans", C.c_double)]


class AtRigtrackResult(C.Structure):
    _fields_ = [("n", C.c_int32), ("with_tags", C.c_int32), ("accepted", C.c_int32), ("rejected", C.c_int32),
                ("cost_before", C.c_double), ("cost_after", C.c_double), ("rms_before", C.c_double),
                ("rms_after", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3), ("cov", C.c_double * 36),
                ("stamp", C.c_double), ("cov_valid", C.c_int32), ("pad", C.c_int32)]


class AtRigtrackInstant(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("stamp", C.c_double), ("rms_px", C.c_double),
                ("n_tags", C.c_int32), ("pad", C.c_int32)]


class AtCamcalConfig(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("init", AtCamera), ("free_mask", C.c_int32),
                ("guess", C.c_int32)]


class AtCamcalResult(C.Structure):
    _fields_ = [("cam", AtCamera), ("cov", C.c_double * 81), ("rms_before", C.c_double), ("rms_after", C.c_double),
                ("views_used", C.c_int32), ("views_skipped", C.c_int32), ("corners", C.c_int32),
                ("accepted", C.c_int32), ("rejected", C.c_int32), ("cov_valid", C.c_int32)]


class AtCamcalView(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("rms_px", C.c_double), ("n_tags", C.c_int32),
                ("used", C.c_int32)]


class AtFieldmapTag(C.Structure):
    _fields_ = [("tag", AtFieldTag), ("known", C.c_int32), ("free_rot", C.c_int32), ("free_trans", C.c_int32),
                ("pad", C.c_int32)]


class AtFieldmapTagResult(C.Structure):
    _fields_ = [("id", C.c_int32), ("placed", C.c_int32), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("R0", C.c_double * 9), ("t0", C.c_double * 3), ("cov", C.c_double * 36), ("views", C.c_int32),
                ("pad", C.c_int32)]


class AtFieldmapResult(C.Structure):
    _fields_ = [("rms_before", C.c_double), ("rms_after", C.c_double), ("views_used", C.c_int32),
                ("views_skipped", C.c_int32), ("corners", C.c_int32), ("accepted", C.c_int32),
                ("rejected", C.c_int32), ("cov_valid", C.c_int32), ("n_tags", C.c_int32), ("n_placed", C.c_int32)]


class AtFieldmapView(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("rms_px", C.c_double), ("n_tags", C.c_int32),
                ("used", C.c_int32)]


class AtQuadRecord(C.Structure):
    _fields_ = [
        ("blob_index", C.c_uint32), ("valid", C.c_uint32), ("accepted", C.c_uint32),
        ("indices", C.c_uint16 * 4), ("corners", (C.c_float * 2) * 4),
    ]


@dataclass
class Detection:
    """apriltag_detection_t fields the node consumes (apriltags_cuda_detector.cu:425-496)."""
    id: int
    hamming: int
    decision_margin: float
    H: np.ndarray
    c: np.ndarray
    p: np.ndarray


@dataclass
class Pose:
    """apriltag_pose_t + the error estimate_tag_pose returns (apriltags_cuda_detector.cu:432-433)."""
    id: int
    R: np.ndarray
    t: np.ndarray
    err: float


@dataclass
class TagDetection:
    """DetectionData of the node loop (apriltags_cuda_detector.cu:425-462): camera- and
    robot-frame position, distance from the camera, pose error."""
    id: int
    camera: np.ndarray
    robot: np.ndarray
    distance: float
    err: float


@dataclass
class FieldPose:
    """at_field_pose: the camera pose of one frame from all its layout tags, x_cam = R x_field + t
    (n_tags == 0: no layout tag in the frame, the rest zero)."""
    n_tags: int
    ids: list
    R: np.ndarray
    t: np.ndarray
    rms_px: float
    steps_taken: int


@dataclass
class RigPose:
    """at_rig_pose: the robot in the field at one instant from the layout tags of every camera of a
    rig, x_field = R x_robot + t, and its covariance in the order (w_x, w_y, w_z, t_x, t_y, t_z) --
    w a small turn in the robot frame, t in the field frame (n_tags == 0: no layout tag in any
    camera, the rest zero)."""
    n_tags: int
    n_cams_used: int
    tags_per_cam: list
    ids: list          # per camera, the ids used (ascending)
    R: np.ndarray
    t: np.ndarray
    cov: np.ndarray    # [6, 6]; zeros unless cov_valid
    cov_valid: bool
    rms_px: float
    steps_taken: int
    rejected: int
    dropped: int


@dataclass
class RigRobust:
    """at_rig_robust_config: corners beyond huber_px are down-weighted (Huber), tags whose corner
    RMS stays beyond reject_px after the fit are dropped and the fit run again, at most max_rounds
    (0..3) times and never below min_keep tags (counted per camera view).  math.inf for both
    thresholds is the plain solve."""
    huber_px: float = 2.0
    reject_px: float = 6.0
    max_rounds: int = 3
    min_keep: int = 2


@dataclass
class RigRobustInfo:
    """at_rig_robust_info of one instant: dropped[c] lists the ids of camera c's selection (the
    RigPose's ids[c]) that were dropped, tag_rms_px[c][j] is the corner RMS of ids[c][j] at the
    final pose (dropped tags included), rounds the number of rounds that dropped tags."""
    n_kept: int
    n_rejected: int
    rounds: int
    starved: bool
    rejected_mask: list
    dropped: list
    tag_rms_px: list
    huber_cost: float
    n_downweighted: int


@dataclass
class RigCalibration:
    """at_rigcal_result: per camera the calibrated extrinsics x_robot = R x_cam + t and the 6 x 6
    covariance of (we, de) -- we a small turn in the camera frame, de in the robot frame; rows and
    columns of parameters that were not free are zero."""
    R: list            # per camera [3, 3]
    t: list            # per camera [3]
    cov: list          # per camera [6, 6]; zeros unless cov_valid
    cov_valid: bool
    rms_before: float
    rms_after: float
    instants_used: int
    instants_skipped: int
    accepted: int
    rejected: int


@dataclass
class RigCalInstant:
    """at_rigcal_instant: a stored instant's final robot pose and RMS (used False: skipped)."""
    R: np.ndarray
    t: np.ndarray
    rms_px: float
    n_tags: int
    used: bool


@dataclass
class RigTrack:
    """at_rigtrack_result: the latest instant's smoothed robot pose x_field = R x_robot + t, its
    6 x 6 covariance in (w, t) order -- w a small turn in the robot frame, t in the field frame --
    and what the solve over the window did."""
    R: np.ndarray      # [3, 3]
    t: np.ndarray      # [3]
    cov: np.ndarray    # [6, 6]; zeros unless cov_valid
    cov_valid: bool
    stamp: float
    n: int
    with_tags: int
    accepted: int
    rejected: int
    cost_before: float
    cost_after: float
    rms_before: float
    rms_after: float


@dataclass
class RigTrackInstant:
    """at_rigtrack_instant: an instant's final robot pose (n_tags 0: held by odometry alone)."""
    R: np.ndarray
    t: np.ndarray
    stamp: float
    rms_px: float
    n_tags: int


@dataclass
class CameraCalibration:
    """at_camcal_result: the calibrated camera as `params` (fx, fy, cx, cy, k1, k2, p1, p2, k3) and its
    9 x 9 covariance in that order; rows and columns of parameters that were not free are zero."""
    params: np.ndarray  # [9]
    cov: np.ndarray     # [9, 9]; zeros unless cov_valid
    cov_valid: bool
    rms_before: float
    rms_after: float
    views_used: int
    views_skipped: int
    corners: int
    accepted: int
    rejected: int

    @property
    def camera_matrix(self):
        return CameraMatrix(fx=float(self.params[0]), cx=float(self.params[2]), fy=float(self.params[1]),
                            cy=float(self.params[3]))

    @property
    def distortion_coefficients(self):
        return DistCoeffs(*[float(x) for x in self.params[4:]])


@dataclass
class CameraCalView:
    """at_camcal_view: the board's final pose in a stored view, x_cam = R x_board + t, and the view's
    RMS (used False: skipped)."""
    R: np.ndarray
    t: np.ndarray
    rms_px: float
    n_tags: int
    used: bool


@dataclass
class FieldMap:
    """at_fieldmap_result: the totals of a field-map solve (the tags are FieldMapper.tags())."""
    rms_before: float
    rms_after: float
    views_used: int
    views_skipped: int
    corners: int
    accepted: int
    rejected: int
    cov_valid: bool
    n_tags: int
    n_placed: int


@dataclass
class FieldMapTag:
    """at_fieldmap_tag_result: a map tag's final pose x_field = R x_tag + t, its start (R0, t0: where
    the caller or the chain of views put it) and the 6 x 6 covariance of (w, d) -- w a small turn in
    the tag frame, d in the field frame; rows and columns of parameters that were not free are
    zero.  placed False: no chain of views reached the tag, the rest is zero."""
    id: int
    placed: bool
    R: np.ndarray
    t: np.ndarray
    R0: np.ndarray
    t0: np.ndarray
    cov: np.ndarray    # [6, 6]; zeros unless the solve's cov_valid
    views: int         # stored views that hold the tag


@dataclass
class FieldMapView:
    """at_fieldmap_view: a stored view's final camera pose, x_cam = R x_field + t, and its RMS
    (used False: skipped)."""
    R: np.ndarray
    t: np.ndarray
    rms_px: float
    n_tags: int
    used: bool


@dataclass
class CameraMatrix:
    """apriltag_gpu.h:61-66"""
    fx: float
    cx: float
    fy: float
    cy: float


@dataclass
class DistCoeffs:
    """apriltag_gpu.h:68-74"""
    k1: float
    k2: float
    p1: float
    p2: float
    k3: float


# Intrinsics the reference's own test uses (test/gpu_detector_test.cu:62-73).
TEST_CAMERA = CameraMatrix(fx=905.495617, cx=609.916016, fy=907.909470, cy=352.682645)
TEST_DIST = DistCoeffs(k1=0.059238, k2=-0.075154, p1=-0.003801, p2=0.001113, k3=0.0)

_LIB = None


def load_library(path: str = LIB_PATH):
    """Load libat_hip.so; raises if it is missing (no CPU fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(path):
        raise RuntimeError("libat_hip.so not built: run `make -C ros_vision_amd/csrc` "
                           "(or __graft_entry__.build())")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7
    # (same soname as /opt/rocm's).  Whichever loads first is the one both use,
    # and torch only initialises on its own copy, so let torch load first when
    # it is installed (it provides device memory / torch.distributed to callers).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    L.at_config_default.argtypes = [C.POINTER(AtConfig), C.c_int, C.c_int]
    L.at_create.argtypes = [C.POINTER(AtConfig), C.POINTER(AtCamera), C.POINTER(C.c_void_p)]
    L.at_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(AtDetection), C.c_int, C.POINTER(C.c_int)]
    L.at_detect_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(AtDetection),
                                  C.c_int, C.POINTER(C.c_int)]
    L.at_detect_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(AtDetection),
                                   C.c_int, C.POINTER(C.c_int)]
    L.at_enqueue_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    if hasattr(L, "at_enqueue_host"):
        L.at_enqueue_host.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int]
    L.at_collect.argtypes = [C.c_void_p, C.POINTER(AtDetection), C.c_int, C.POINTER(C.c_int)]
    L.at_stream_wait.argtypes = [C.c_void_p, C.c_void_p]
    L.at_frame_status.argtypes = [C.c_void_p, C.c_int]
    L.at_debug_copy.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.at_debug_copy.restype = C.c_longlong
    L.at_destroy.argtypes = [C.c_void_p]
    L.at_strerror.restype = C.c_char_p
    L.at_strerror.argtypes = [C.c_int]
    L.at_family_num_known.argtypes = [C.c_char_p]
    L.at_family_entry.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    L.at_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.at_stage_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    L.at_stage_name.restype = C.c_char_p
    L.at_stage_name.argtypes = [C.c_int]
    L.at_poses.argtypes = [C.c_void_p, C.c_int, C.POINTER(AtPose), C.c_int]
    L.at_set_kernel_timer.argtypes = [C.c_void_p, C.c_int]
    L.at_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    if hasattr(L, "at_kernel_span"):
        L.at_kernel_span.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.at_batch_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    L.at_tag_detections.argtypes = [C.POINTER(AtPose), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(AtTagDetection)]
    if hasattr(L, "at_set_debug_taps"):
        L.at_set_debug_taps.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "at_gp_enable"):  # (A/B builds of older sources lack it)
        L.at_gp_enable.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.at_gp_tensor.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.at_gp_copy.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.at_gp_preprocess_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p]
    if hasattr(L, "at_draw_outlines_device"):
        L.at_draw_outlines_device.argtypes = [C.c_void_p, C.POINTER(AtDetection), C.c_int, C.c_void_p]
    if hasattr(L, "at_detections"):  # (A/B builds of older sources lack them)
        L.at_detections.argtypes = [C.c_void_p, C.c_int, C.POINTER(AtDetection), C.c_int]
        L.at_annotate_staged.argtypes = [C.c_void_p, C.c_int, C.POINTER(AtDetection), C.c_int, C.c_void_p]
    if hasattr(L, "at_enqueue_mjpg"):  # (A/B builds of older sources lack the MJPG path)
        L.at_enqueue_mjpg.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int,
                                      C.POINTER(C.c_int)]
        L.at_detect_mjpg.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(AtDetection), C.c_int,
                                     C.POINTER(C.c_int)]
        L.at_detect_mjpg_batch.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int,
                                           C.POINTER(AtDetection), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.at_mjpg_set_threads.argtypes = [C.c_void_p, C.c_int]
        L.at_mjpg_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.at_mjpg_decode_gray_host.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                               C.POINTER(C.c_int)]
        L.at_mjpg_stream_mode_host.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    if hasattr(L, "at_mjpg_set_color"):  # (A/B builds of older sources lack the colour path)
        L.at_mjpg_set_color.argtypes = [C.c_void_p, C.c_int]
        L.at_mjpg_bgr.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.at_mjpg_copy_bgr.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.at_mjpg_decode_bgr_host.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                              C.POINTER(C.c_int)]
    if hasattr(L, "at_mjpg_set_device_entropy"):  # (A/B builds of older sources lack the device entropy decode)
        L.at_mjpg_set_device_entropy.argtypes = [C.c_void_p, C.c_int]
        L.at_mjpg_set_subseq.argtypes = [C.c_void_p, C.c_int]
        L.at_mjpg_entropy_host.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_size_t, C.POINTER(C.c_int)]
        L.at_mjpg_dense_host.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]
    if hasattr(L, "at_annotate_jpeg"):  # (A/B builds of older sources lack the JPEG output)
        L.at_encode_jpeg_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_size_t)]
        L.at_annotate_jpeg.argtypes = [C.c_void_p, C.c_int, C.POINTER(AtDetection), C.c_int, C.c_int, C.c_int,
                                       C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.at_jpeg_max_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.at_jpeg_max_bytes.restype = C.c_size_t
        L.at_jpeg_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.at_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        L.at_host_free.argtypes = [C.c_void_p]
        L.at_host_free.restype = None
        L.at_jpeg_encode_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_size_t)]
    if hasattr(L, "at_gp_parse_host"):  # (A/B builds of older sources lack the output parse)
        L.at_gp_parse_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int,
                                       C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.at_gp_parse_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_float,
                                         C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.at_gp_draw_boxes_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.at_gp_parse_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.at_gp_annotate_staged.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.at_gp_annotate_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                          C.c_size_t, C.POINTER(C.c_size_t)]
        L.at_gp_copy_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    if hasattr(L, "at_preview_jpeg"):  # (A/B builds of older sources lack the preview stream)
        ip = C.POINTER(C.c_int)
        recs = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]  # at_detection records, boxes
        jpeg_tail = [C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), ip]
        L.at_preview_size.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, ip]
        L.at_preview_bgr.argtypes = [C.c_void_p, C.c_int, C.c_int] + recs + [C.c_void_p]
        L.at_preview_jpeg.argtypes = [C.c_void_p, C.c_int, C.c_int] + recs + jpeg_tail
        L.at_preview_jpeg_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + recs + jpeg_tail
        L.at_preview_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + recs + [C.c_void_p, C.c_size_t]
        L.at_preview_jpeg_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + recs + jpeg_tail
        L.at_preview_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    if hasattr(L, "at_field_poses"):  # (A/B builds of older sources lack the field pose)
        dp = C.POINTER(C.c_double)
        L.at_set_field_layout.argtypes = [C.c_void_p, C.POINTER(AtFieldTag), C.c_int, C.c_int]
        L.at_field_poses.argtypes = [C.c_void_p, C.POINTER(AtFieldPose), C.c_int]
        L.at_field_pose_host.argtypes = [C.POINTER(AtDetection), C.POINTER(AtPose), C.c_int, C.POINTER(AtFieldTag),
                                         C.c_int, C.c_int, C.POINTER(AtCamera), C.c_double, C.POINTER(AtFieldPose)]
        L.at_robot_in_field.argtypes = [C.POINTER(AtFieldPose), dp, dp, dp, dp]
        L.at_field_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    if hasattr(L, "at_rig_solve"):  # (A/B builds of older sources lack the rig pose)
        L.at_rig_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(AtRigExtrinsics), C.c_int, C.POINTER(AtFieldTag),
                                    C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.at_rig_solve.argtypes = [C.c_void_p, C.POINTER(AtRigPose), C.c_int]
        L.at_rig_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.at_rig_destroy.argtypes = [C.c_void_p]
        L.at_rig_destroy.restype = None
        L.at_rig_pose_host.argtypes = [C.POINTER(AtRigHostCam), C.c_int, C.POINTER(AtFieldTag), C.c_int, C.c_int,
                                       C.c_double, C.POINTER(AtRigPose)]
    if hasattr(L, "at_rig_solve_robust"):  # (A/B builds of older sources lack the robust rig pose)
        L.at_rig_solve_robust.argtypes = [C.c_void_p, C.POINTER(AtRigRobustConfig), C.POINTER(AtRigPose),
                                          C.POINTER(AtRigRobustInfo), C.c_int]
        L.at_rig_pose_robust_host.argtypes = [C.POINTER(AtRigHostCam), C.c_int, C.POINTER(AtFieldTag), C.c_int, C.c_int,
                                              C.c_double, C.POINTER(AtRigRobustConfig), C.POINTER(AtRigPose),
                                              C.POINTER(AtRigRobustInfo)]
        L.at_rig_robust_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    if hasattr(L, "at_rigcal_solve"):  # (A/B builds of older sources lack the rig calibration)
        L.at_rigcal_create.argtypes = [C.POINTER(AtRigcalCamera), C.c_int, C.POINTER(AtFieldTag), C.c_int, C.c_int,
                                       C.c_double, C.POINTER(C.c_void_p)]
        L.at_rigcal_add.argtypes = [C.c_void_p, C.POINTER(AtRigcalFrame)]
        for name in ("at_rigcal_count", "at_rigcal_clear"):
            getattr(L, name).argtypes = [C.c_void_p]
        for name in ("at_rigcal_solve", "at_rigcal_solve_host"):
            getattr(L, name).argtypes = [C.c_void_p, C.POINTER(AtRigcalResult)]
        L.at_rigcal_instants.argtypes = [C.c_void_p, C.POINTER(AtRigcalInstant), C.c_int]
        L.at_rigcal_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.at_rigcal_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.at_rigcal_destroy.argtypes = [C.c_void_p]
        L.at_rigcal_destroy.restype = None
    if hasattr(L, "at_rigtrack_solve"):  # (A/B builds of older sources lack the rig track)
        L.at_rigtrack_create.argtypes = [C.POINTER(AtRigtrackCamera), C.c_int, C.POINTER(AtFieldTag), C.c_int, C.c_int,
                                         C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.at_rigtrack_push.argtypes = [C.c_void_p, C.c_double, C.POINTER(AtRigcalFrame), C.POINTER(AtRigtrackOdom)]
        for name in ("at_rigtrack_count", "at_rigtrack_clear"):
            getattr(L, name).argtypes = [C.c_void_p]
        for name in ("at_rigtrack_solve", "at_rigtrack_solve_host"):
            getattr(L, name).argtypes = [C.c_void_p, C.POINTER(AtRigtrackResult)]
        L.at_rigtrack_instants.argtypes = [C.c_void_p, C.POINTER(AtRigtrackInstant), C.c_int]
        L.at_rigtrack_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.at_rigtrack_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.at_rigtrack_destroy.argtypes = [C.c_void_p]
        L.at_rigtrack_destroy.restype = None
    if hasattr(L, "at_camcal_solve"):  # (A/B builds of older sources lack the camera calibration)
        L.at_camcal_create.argtypes = [C.POINTER(AtCamcalConfig), C.POINTER(AtFieldTag), C.c_int, C.c_int, C.c_double,
                                       C.POINTER(C.c_void_p)]
        L.at_camcal_add.argtypes = [C.c_void_p, C.POINTER(AtDetection), C.c_int]
        for name in ("at_camcal_count", "at_camcal_clear"):
            getattr(L, name).argtypes = [C.c_void_p]
        for name in ("at_camcal_solve", "at_camcal_solve_host"):
            getattr(L, name).argtypes = [C.c_void_p, C.POINTER(AtCamcalResult)]
        L.at_camcal_views.argtypes = [C.c_void_p, C.POINTER(AtCamcalView), C.c_int]
        L.at_camcal_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.at_camcal_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.at_camcal_destroy.argtypes = [C.c_void_p]
        L.at_camcal_destroy.restype = None
    if hasattr(L, "at_fieldmap_solve"):  # (A/B builds of older sources lack the field map)
        L.at_fieldmap_create.argtypes = [C.POINTER(AtFieldmapTag), C.c_int, C.c_int, C.c_double, C.POINTER(C.c_void_p)]
        L.at_fieldmap_add.argtypes = [C.c_void_p, C.POINTER(AtDetection), C.POINTER(AtPose), C.c_int,
                                      C.POINTER(AtCamera)]
        for name in ("at_fieldmap_count", "at_fieldmap_clear"):
            getattr(L, name).argtypes = [C.c_void_p]
        for name in ("at_fieldmap_solve", "at_fieldmap_solve_host"):
            getattr(L, name).argtypes = [C.c_void_p, C.POINTER(AtFieldmapResult)]
        L.at_fieldmap_tags.argtypes = [C.c_void_p, C.POINTER(AtFieldmapTagResult), C.c_int]
        L.at_fieldmap_views.argtypes = [C.c_void_p, C.POINTER(AtFieldmapView), C.c_int]
        L.at_fieldmap_set_profiling.argtypes = [C.c_void_p, C.c_int]
        L.at_fieldmap_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.at_fieldmap_destroy.argtypes = [C.c_void_p]
    if hasattr(L, "at_set_undistort"):  # (A/B builds of older sources lack the ideal corners)
        dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        L.at_set_undistort.argtypes = [C.c_void_p, C.c_int]
        L.at_ideal_detections.argtypes = [C.c_void_p, C.c_int, C.POINTER(AtDetection), C.c_int]
        L.at_ideal_detections_host.argtypes = [C.POINTER(AtCamera), C.POINTER(AtDetection), C.c_int,
                                               C.POINTER(AtDetection)]
        L.at_undistort_points.argtypes = [C.c_void_p, dp, C.c_int, dp, bp]
        L.at_undistort_points_host.argtypes = [C.POINTER(AtCamera), dp, C.c_int, dp, bp]
        L.at_undistort_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
        L.at_fieldmap_destroy.restype = None
    _LIB = L
    return L


class MjpgError(RuntimeError):
    """An MJPG frame the library refused: `code` is AT_E_UNSUPPORTED or AT_E_INVALID,
    `frame` its index in the batch (None for the host-only calls)."""

    def __init__(self, what, code, frame=None):
        where = "" if frame is None else " (frame %d)" % frame
        super().__init__("%s failed%s: %s (%d)" % (what, where, load_library().at_strerror(code).decode(), code))
        self.code, self.frame = code, frame


def mjpg_decode_gray(jpg: bytes):
    """at_mjpg_decode_gray_host: the luma plane (H, W) uint8 of one baseline JPEG,
    decoded on the host with the integer IDCT k_mjpg_idct runs (no device needed)."""
    L = load_library()
    jpg = bytes(jpg)
    w, h = C.c_int(), C.c_int()
    rc = L.at_mjpg_decode_gray_host(jpg, len(jpg), None, 0, C.byref(w), C.byref(h))
    if rc < 0:
        raise MjpgError("at_mjpg_decode_gray_host", rc)
    out = np.empty((h.value, w.value), np.uint8)
    rc = L.at_mjpg_decode_gray_host(jpg, len(jpg), out.ctypes.data, out.size, C.byref(w), C.byref(h))
    if rc < 0:
        raise MjpgError("at_mjpg_decode_gray_host", rc)
    return out


def mjpg_decode_bgr(jpg: bytes):
    """at_mjpg_decode_bgr_host: the BGR8 image (H, W, 3) uint8 of one baseline JPEG, decoded
    on the host with the arithmetic the colour kernels run (no device needed): libjpeg's
    integer IDCT, fancy upsampling and colour conversion."""
    L = load_library()
    jpg = bytes(jpg)
    w, h = C.c_int(), C.c_int()
    rc = L.at_mjpg_decode_bgr_host(jpg, len(jpg), None, 0, C.byref(w), C.byref(h))
    if rc < 0:
        raise MjpgError("at_mjpg_decode_bgr_host", rc)
    out = np.empty((h.value, w.value, 3), np.uint8)
    rc = L.at_mjpg_decode_bgr_host(jpg, len(jpg), out.ctypes.data, out.size, C.byref(w), C.byref(h))
    if rc < 0:
        raise MjpgError("at_mjpg_decode_bgr_host", rc)
    return out


class JpegError(RuntimeError):
    """A JPEG encode the library refused: `code` is AT_E_INVALID (quality, sampling, size,
    gating) or AT_E_CAPACITY (then `needed` is the stream's size)."""

    def __init__(self, what, code, needed=0):
        super().__init__("%s failed: %s (%d)" % (what, load_library().at_strerror(code).decode(), code))
        self.code, self.needed = code, needed


def _jpeg_sampling(sampling):
    if sampling not in JPEG_SAMPLINGS:
        raise JpegError("JPEG encode (sampling %r)" % (sampling,), AT_E_INVALID)
    return JPEG_SAMPLINGS[sampling]


def jpeg_max_bytes(width: int, height: int, sampling="4:2:0"):
    """at_jpeg_max_bytes: a capacity no JPEG of this geometry exceeds."""
    return int(load_library().at_jpeg_max_bytes(int(width), int(height), _jpeg_sampling(sampling)))


def jpeg_encode_host(bgr, quality=95, sampling="4:2:0", cap=None):
    """at_jpeg_encode_host: the BGR8 image (H, W, 3), H and W multiples of 8, as a baseline
    JPEG (bytes), encoded on the host with the arithmetic the encode kernels run (no device
    needed): byte for byte libjpeg's stream with one restart interval per MCU row."""
    L = load_library()
    bgr = np.ascontiguousarray(bgr, np.uint8)
    if bgr.ndim != 3 or bgr.shape[2] != 3:
        raise JpegError("at_jpeg_encode_host", AT_E_INVALID)
    h, w = bgr.shape[:2]
    s = _jpeg_sampling(sampling)
    if cap is None:
        cap = int(L.at_jpeg_max_bytes(w, h, s))
    out = np.empty(max(int(cap), 1), np.uint8)
    n = C.c_size_t()
    rc = L.at_jpeg_encode_host(bgr.ctypes.data, w, h, int(quality), s, out.ctypes.data, int(cap), C.byref(n))
    if rc < 0:
        raise JpegError("at_jpeg_encode_host", rc, n.value)
    return out[:n.value].tobytes()


def preview_size(width: int, height: int, scale: int):
    """at_preview_size: (pw, ph, ox, oy) of the preview of a width x height frame at integer
    `scale` 1..8 -- pw = (width // scale) & ~7, the crop centred.  JpegError (AT_E_INVALID)
    for a scale outside 1..8 or a preview under 8 x 8."""
    v = [C.c_int() for _ in range(4)]
    rc = load_library().at_preview_size(int(width), int(height), int(scale), *[C.byref(x) for x in v])
    if rc < 0:
        raise JpegError("at_preview_size", rc)
    return tuple(x.value for x in v)


def _box_records(boxes):
    """GP_BOX_DTYPE records of GamePieceBox objects / records / None."""
    if boxes is None:
        return np.empty(0, GP_BOX_DTYPE)
    if isinstance(boxes, np.ndarray) and boxes.dtype == GP_BOX_DTYPE:
        return np.ascontiguousarray(boxes)
    return np.array([(b.x, b.y, b.w, b.h, b.conf, b.cls) for b in boxes], GP_BOX_DTYPE)


def _detection_records(dets):
    """An AtDetection array of AtDetection records or Detection objects, and its length."""
    dets = list(dets or ())
    arr = (AtDetection * max(1, len(dets)))()
    for i, d in enumerate(dets):
        if isinstance(d, AtDetection):
            arr[i] = d
            continue
        arr[i].id, arr[i].hamming, arr[i].decision_margin = int(d.id), int(d.hamming), float(d.decision_margin)
        for k, v in enumerate(np.asarray(d.H, np.float64).reshape(9)):
            arr[i].H[k] = v
        arr[i].c[0], arr[i].c[1] = float(d.c[0]), float(d.c[1])
        for k in range(4):
            arr[i].p[k][0], arr[i].p[k][1] = float(d.p[k][0]), float(d.p[k][1])
    return arr, len(dets)


def _preview_frame(frame, fmt):
    """(contiguous uint8 frame, width, height) of a frame shaped as the detector takes it."""
    frame = np.ascontiguousarray(frame, np.uint8)
    h = frame.shape[0]
    if fmt == AT_FMT_BGR8:
        w = frame.shape[1]
    elif fmt == AT_FMT_YUYV:
        w = frame.shape[1] if frame.ndim == 3 else frame.shape[1] // 2
    else:
        w = frame.shape[1]
    return frame, w, h


def preview_host(frame, fmt, scale, detections=None, boxes=None):
    """at_preview_host: the CPU reference of GpuDetector.preview_bgr (no device needed).
    `frame`: (H, W, 3) BGR8, (H, W, 2) or (H, 2 W) YUYV, (H, W) GRAY8; `detections`:
    Detection objects or at_detection records; `boxes`: GamePieceBox objects or records.
    Returns the annotated preview (ph, pw, 3) uint8."""
    L = load_library()
    frame, w, h = _preview_frame(frame, fmt)
    pw, ph, _, _ = preview_size(w, h, scale)
    arr, n = _detection_records(detections)
    rec = _box_records(boxes)
    out = np.empty((ph, pw, 3), np.uint8)
    rc = L.at_preview_host(frame.ctypes.data, fmt, w, h, int(scale), C.addressof(arr), n,
                           rec.ctypes.data if len(rec) else None, len(rec), out.ctypes.data, out.size)
    if rc < 0:
        raise JpegError("at_preview_host", rc)
    return out


def preview_jpeg_host(frame, fmt, scale, detections=None, boxes=None, quality=50, sampling="4:2:0", max_bytes=0,
                      cap=None):
    """at_preview_jpeg_host: the CPU reference of GpuDetector.preview_jpeg: (bytes, quality
    used).  JpegError with code AT_E_CAPACITY, `needed` and `quality_used` when the stream
    exceeds `cap` or no quality fits `max_bytes`."""
    L = load_library()
    frame, w, h = _preview_frame(frame, fmt)
    pw, ph, _, _ = preview_size(w, h, scale)
    s = _jpeg_sampling(sampling)
    if cap is None:
        cap = int(L.at_jpeg_max_bytes(pw, ph, s))
    arr, n = _detection_records(detections)
    rec = _box_records(boxes)
    out = np.empty(max(int(cap), 1), np.uint8)
    ln, qu = C.c_size_t(), C.c_int()
    rc = L.at_preview_jpeg_host(frame.ctypes.data, fmt, w, h, int(scale), C.addressof(arr), n,
                                rec.ctypes.data if len(rec) else None, len(rec), int(quality), s, int(max_bytes),
                                out.ctypes.data, int(cap), C.byref(ln), C.byref(qu))
    if rc < 0:
        e = JpegError("at_preview_jpeg_host", rc, ln.value)
        e.quality_used = qu.value
        raise e
    return out[:ln.value].tobytes(), qu.value


def mjpg_stream_mode(jpg: bytes, width: int = 0, height: int = 0):
    """at_mjpg_stream_mode_host: ("sparse" | "dense", bytes on the link) of one frame on
    its way to a width x height detector (0, 0: any size); raises MjpgError with the
    code at_enqueue_mjpg would return for it."""
    L = load_library()
    jpg = bytes(jpg)
    n = C.c_size_t()
    rc = L.at_mjpg_stream_mode_host(jpg, len(jpg), int(width), int(height), C.byref(n))
    if rc < 0:
        raise MjpgError("at_mjpg_stream_mode_host", rc)
    return ("dense" if rc else "sparse"), n.value


def mjpg_dense_host(jpg: bytes, width: int = 0, height: int = 0, keep_chroma=False):
    """at_mjpg_dense_host: the frame's coefficient streams as the serial host decoder gives
    them, every plane dense (uint8 array: headers and payloads, the layout of at_mjpg.h)."""
    L = load_library()
    jpg = bytes(jpg)
    n = C.c_size_t()
    rc = L.at_mjpg_dense_host(jpg, len(jpg), int(width), int(height), int(bool(keep_chroma)), None, 0, C.byref(n))
    if rc < 0:
        raise MjpgError("at_mjpg_dense_host", rc)
    out = np.empty(n.value, np.uint8)
    rc = L.at_mjpg_dense_host(jpg, len(jpg), int(width), int(height), int(bool(keep_chroma)), out.ctypes.data,
                              out.size, C.byref(n))
    if rc < 0:
        raise MjpgError("at_mjpg_dense_host", rc)
    return out


def mjpg_entropy_host(jpg: bytes, subseq_bytes: int, width: int = 0, height: int = 0, keep_chroma=False, nbytes=None):
    """at_mjpg_entropy_host: the same streams from the parallel subsequence algorithm of
    k_mjpg_entropy, run on the host piece by piece -> (uint8 array, rounds).  `nbytes`: the
    streams' size where the caller knows it (else the serial decoder is asked)."""
    L = load_library()
    jpg = bytes(jpg)
    if nbytes is None:
        n = C.c_size_t()
        rc = L.at_mjpg_dense_host(jpg, len(jpg), int(width), int(height), int(bool(keep_chroma)), None, 0,
                                  C.byref(n))
        if rc < 0:
            raise MjpgError("at_mjpg_dense_host", rc)
        nbytes = n.value
    out = np.empty(int(nbytes), np.uint8)
    rounds = C.c_int()
    rc = L.at_mjpg_entropy_host(jpg, len(jpg), int(width), int(height), int(subseq_bytes), int(bool(keep_chroma)),
                                out.ctypes.data, out.size, C.byref(rounds))
    if rc < 0:
        raise MjpgError("at_mjpg_entropy_host", rc)
    return out, rounds.value


def game_piece_preprocess_device(bgr_ptr: int, width: int, height: int, out_ptr: int, out_width: int = 640,
                                 out_height: int = 640, channels: int = 3, stream: int = 0):
    """at_gp_preprocess_device: preprocess_image of one device-resident BGR8 image
    into a device NCHW float buffer, enqueued on `stream` (hipStream_t handle)."""
    _check(load_library().at_gp_preprocess_device(bgr_ptr, width, height, out_ptr, out_width, out_height, channels,
                                                  stream or None), "at_gp_preprocess_device")


@dataclass
class GamePieceBox:
    """YoloDetection (yolo_detection.h:13-48) after scale_detections: centre, size in camera
    pixels, confidence, class (and its name where the node knows the model's class names)."""
    x: float
    y: float
    w: float
    h: float
    conf: float
    cls: int
    class_name: str = ""


class GamePieceCapacityError(RuntimeError):
    """game_piece_parse: `frame` had more than AT_GP_MAX_CANDIDATES candidates."""

    def __init__(self, frame):
        super().__init__("at_gp_parse_device: frame %d exceeded %d candidates (AT_E_CAPACITY)"
                         % (frame, AT_GP_MAX_CANDIDATES))
        self.frame, self.code = frame, AT_E_CAPACITY


def game_piece_boxes(records, class_names=()):
    """GP_BOX_DTYPE records -> [GamePieceBox]."""
    names = list(class_names)
    return [GamePieceBox(float(r["x"]), float(r["y"]), float(r["w"]), float(r["h"]), float(r["conf"]), int(r["cls"]),
                         names[int(r["cls"])] if 0 <= int(r["cls"]) < len(names) else ("unknown" if names else ""))
            for r in records]


def _gp_parse_host_frame(raw, conf, iou, model_size, orig_size, cap=None):
    L = load_library()
    c4, p = raw.shape
    n = C.c_int()
    args = (raw.ctypes.data, p, c4 - 4, conf, iou, int(model_size[0]), int(model_size[1]), int(orig_size[0]),
            int(orig_size[1]))
    if cap is None:
        _check(L.at_gp_parse_host(*args, None, 0, C.byref(n)), "at_gp_parse_host")
        cap = n.value
    out = np.zeros(max(int(cap), 1), GP_BOX_DTYPE)
    _check(L.at_gp_parse_host(*args, out.ctypes.data, int(cap), C.byref(n)), "at_gp_parse_host")
    return out[:min(n.value, int(cap))], n.value


def game_piece_parse_host(raw, conf=0.25, iou=0.45, model_size=(640, 640), orig_size=None, records=False):
    """at_gp_parse_host: the reference node's parse_yolov11_output + apply_nms +
    scale_detections of a network output `raw`, [4 + C, P] or [B, 4 + C, P] float32, on the
    host (no device needed) -- the CPU reference of GpuDetector.game_piece_parse.
    model_size / orig_size are (width, height); orig_size None leaves model coordinates.
    Returns the boxes in NMS order ([GamePieceBox], or GP_BOX_DTYPE records with
    records=True); one list per frame for a 3-D `raw`."""
    raw = np.ascontiguousarray(raw, np.float32)
    orig_size = model_size if orig_size is None else orig_size
    if raw.ndim not in (2, 3) or raw.shape[-2] < 5 or raw.shape[-1] < 1:
        raise RuntimeError("at_gp_parse_host failed: raw must be [4 + C, P] or [B, 4 + C, P] (%d)" % AT_E_INVALID)
    frames = raw[None] if raw.ndim == 2 else raw
    res = []
    for fr in frames:
        rec, _ = _gp_parse_host_frame(fr, conf, iou, model_size, orig_size)
        res.append(rec if records else game_piece_boxes(rec))
    return res[0] if raw.ndim == 2 else res


def family_entries(family: str = "tag36h11"):
    """(id, code) pairs of the codewords known to the library."""
    L = load_library()
    n = L.at_family_num_known(family.encode())
    out = []
    for i in range(n):
        tid, code = C.c_int(), C.c_uint64()
        L.at_family_entry(family.encode(), i, C.byref(tid), C.byref(code))
        out.append((tid.value, code.value))
    return out


def tag_detections(poses, extrinsic_rotation=None, extrinsic_offset=None):
    """The node's per-frame tail (apriltags_cuda_detector.cu:425-462, 595-599):
    transformCameraToRobot + distance, sorted closest first.  Runs in libat_hip.so
    (host code, no device needed)."""
    L = load_library()
    n = len(poses)
    arr = (AtPose * max(1, n))()
    for i, p in enumerate(poses):
        arr[i].id = int(p.id)
        arr[i].R[:] = [float(x) for x in np.asarray(p.R, np.float64).ravel()]
        arr[i].t[:] = [float(x) for x in np.asarray(p.t, np.float64).ravel()]
        arr[i].err = float(p.err)
    Rp = tp = None
    if extrinsic_rotation is not None:
        Rv = np.ascontiguousarray(extrinsic_rotation, np.float64).reshape(9)
        Rp = Rv.ctypes.data_as(C.POINTER(C.c_double))
    if extrinsic_offset is not None:
        tv = np.ascontiguousarray(extrinsic_offset, np.float64).reshape(3)
        tp = tv.ctypes.data_as(C.POINTER(C.c_double))
    out = (AtTagDetection * max(1, n))()
    _check(L.at_tag_detections(arr, n, Rp, tp, out), "at_tag_detections")
    return [TagDetection(id=o.id, camera=np.array(list(o.camera)), robot=np.array(list(o.robot)),
                         distance=o.distance, err=o.err) for o in out[:n]]


class FieldPoseError(RuntimeError):
    """A field-pose call the library refused; `code` is the AT_E_* value (AT_E_INVALID: a bad
    layout, tag_size 0, a batch not yet collected, a record without tags)."""

    def __init__(self, what, code):
        super().__init__("%s failed: %s (%d)" % (what, load_library().at_strerror(code).decode(), code))
        self.code = code


def _field_tags(tags):
    """A layout -- (id, R, t) triples -- as at_field_tag records."""
    tags = list(tags or ())
    arr = (AtFieldTag * max(1, len(tags)))()
    for i, (tid, R, t) in enumerate(tags):
        arr[i].id = int(tid)
        arr[i].R[:] = [float(x) for x in np.asarray(R, np.float64).reshape(9)]
        arr[i].t[:] = [float(x) for x in np.asarray(t, np.float64).reshape(3)]
    return arr, len(tags)


def _field_pose(o):
    return FieldPose(n_tags=o.n_tags, ids=[int(x) for x in o.ids[:o.n_tags]], R=np.array(list(o.R)).reshape(3, 3),
                     t=np.array(list(o.t)), rms_px=o.rms_px, steps_taken=o.steps_taken)


def _field_pose_record(fp):
    o = AtFieldPose()
    o.n_tags = int(fp.n_tags)
    for i, tid in enumerate(fp.ids):
        o.ids[i] = int(tid)
    o.R[:] = [float(x) for x in np.asarray(fp.R, np.float64).reshape(9)]
    o.t[:] = [float(x) for x in np.asarray(fp.t, np.float64).reshape(3)]
    o.rms_px, o.steps_taken = float(fp.rms_px), int(fp.steps_taken)
    return o


def field_pose_host(detections, poses, tags, max_hamming=0, camera_matrix=None, tag_size=TAG_SIZE):
    """at_field_pose_host: the field pose of one frame on the CPU, from its detections() and
    poses() (same order) and a layout of (id, R, t) triples -- the reference the GPU path
    (GpuDetector.field_poses) is held to.  Raises FieldPoseError for a layout or tag_size the
    library refuses."""
    L = load_library()
    cam = camera_matrix or TEST_CAMERA
    if len(detections) != len(poses):
        raise ValueError("one pose per detection")
    (darr, n), tarr_n = _detection_records(detections), _field_tags(tags)
    parr = (AtPose * max(1, n))()
    for i, p in enumerate(poses):
        parr[i].id = int(p.id)
        parr[i].R[:] = [float(x) for x in np.asarray(p.R, np.float64).reshape(9)]
        parr[i].t[:] = [float(x) for x in np.asarray(p.t, np.float64).reshape(3)]
        parr[i].err = float(p.err)
    c = AtCamera(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
    out = AtFieldPose()
    rc = L.at_field_pose_host(darr, parr, n, tarr_n[0], tarr_n[1], int(max_hamming), C.byref(c), float(tag_size),
                              C.byref(out))
    if rc < 0:
        raise FieldPoseError("at_field_pose_host", rc)
    return _field_pose(out)


# ---- ideal corners (at_undist.h) ---------------------------------------------------
def _at_camera(camera_matrix, distortion_coefficients):
    cam, dist = camera_matrix or TEST_CAMERA, distortion_coefficients or TEST_DIST
    return AtCamera(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, k1=dist.k1, k2=dist.k2, p1=dist.p1, p2=dist.p2,
                    k3=dist.k3)


def _detections_of(records):
    return [Detection(id=d.id, hamming=d.hamming, decision_margin=d.decision_margin,
                      H=np.array(list(d.H)).reshape(3, 3), c=np.array(list(d.c)),
                      p=np.array([[d.p[k][0], d.p[k][1]] for k in range(4)])) for d in records]


def ideal_detections_host(detections, camera_matrix=None, distortion_coefficients=None):
    """at_ideal_detections_host: the detections with H, c and p from ideal corners -- the lens
    distortion undone by the exact inverse of the forward model -- and id = -1 (raw values) where
    a corner is not invertible; on the CPU, bit-equal to GpuDetector.ideal_detections."""
    arr, n = _detection_records(detections)
    out = (AtDetection * max(1, n))()
    c = _at_camera(camera_matrix, distortion_coefficients)
    _check(load_library().at_ideal_detections_host(C.byref(c), arr, n, out), "at_ideal_detections_host")
    return _detections_of(out[:n])


def _points_in(xy):
    xy = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
    return xy, np.empty_like(xy), np.zeros(len(xy), np.uint8)


def undistort_points_host(xy, camera_matrix=None, distortion_coefficients=None):
    """at_undistort_points_host: (n, 2) raw pixels -> ((n, 2) ideal pixels, (n,) bool ok); a pixel
    that is not invertible comes back raw with ok False.  Bit-equal to GpuDetector.undistort_points."""
    xy, out, ok = _points_in(xy)
    c = _at_camera(camera_matrix, distortion_coefficients)
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    _check(load_library().at_undistort_points_host(C.byref(c), xy.ctypes.data_as(dp), len(xy), out.ctypes.data_as(dp),
                                                   ok.ctypes.data_as(bp)), "at_undistort_points_host")
    return out, ok.astype(bool)


def robot_in_field(field_pose, extrinsic_rotation=None, extrinsic_offset=None):
    """at_robot_in_field: (R, t) of the robot in the field, field_T_cam (robot_T_cam)^-1, from a
    FieldPose and the camera -> robot extrinsics tag_detections takes.  Host only."""
    Rp = tp = None
    dp = C.POINTER(C.c_double)
    if extrinsic_rotation is not None:
        Rv = np.ascontiguousarray(extrinsic_rotation, np.float64).reshape(9)
        Rp = Rv.ctypes.data_as(dp)
    if extrinsic_offset is not None:
        tv = np.ascontiguousarray(extrinsic_offset, np.float64).reshape(3)
        tp = tv.ctypes.data_as(dp)
    R, t = np.empty(9), np.empty(3)
    rec = _field_pose_record(field_pose)
    rc = load_library().at_robot_in_field(C.byref(rec), Rp, tp, R.ctypes.data_as(dp), t.ctypes.data_as(dp))
    if rc < 0:
        raise FieldPoseError("at_robot_in_field", rc)
    return R.reshape(3, 3), t


# ---- rig pose (k_rig) ---------------------------------------------------------
def _rig_pose(o):
    return RigPose(n_tags=o.n_tags, n_cams_used=o.n_cams_used, tags_per_cam=[int(x) for x in o.tags_per_cam],
                   ids=[[int(x) for x in o.ids[i][:o.tags_per_cam[i]]] for i in range(AT_RIG_MAX_CAMS)],
                   R=np.array(list(o.R)).reshape(3, 3), t=np.array(list(o.t)), cov=np.array(list(o.cov)).reshape(6, 6),
                   cov_valid=bool(o.cov_valid), rms_px=o.rms_px, steps_taken=o.steps_taken, rejected=o.rejected,
                   dropped=o.dropped)


def _rig_extrinsics(extrinsics, n):
    """(R, t) pairs, x_robot = R x_cam + t (None: identity / zero), as at_rig_extrinsics records."""
    extrinsics = list(extrinsics) if extrinsics is not None else [None] * n
    arr = (AtRigExtrinsics * max(1, len(extrinsics)))()
    for i, e in enumerate(extrinsics):
        R, t = (np.eye(3), np.zeros(3)) if e is None else e
        arr[i].R[:] = [float(x) for x in np.asarray(np.eye(3) if R is None else R, np.float64).reshape(9)]
        arr[i].t[:] = [float(x) for x in np.asarray(np.zeros(3) if t is None else t, np.float64).reshape(3)]
    return arr, len(extrinsics)


def _rig_robust_config(cfg):
    """The at_rig_robust_config of a RigRobust (None: a NULL pointer, which the library refuses)."""
    if cfg is None:
        return None
    return AtRigRobustConfig(huber_px=float(cfg.huber_px), reject_px=float(cfg.reject_px),
                             max_rounds=int(cfg.max_rounds), min_keep=int(cfg.min_keep))


def _rig_robust_info(o, pose):
    masks = [int(x) for x in o.rejected_mask]
    return RigRobustInfo(n_kept=o.n_kept, n_rejected=o.n_rejected, rounds=o.rounds, starved=bool(o.starved),
                         rejected_mask=masks,
                         dropped=[[i for j, i in enumerate(pose.ids[c]) if masks[c] >> j & 1]
                                  for c in range(AT_RIG_MAX_CAMS)],
                         tag_rms_px=[[float(x) for x in o.tag_rms_px[c][:pose.tags_per_cam[c]]]
                                     for c in range(AT_RIG_MAX_CAMS)],
                         huber_cost=o.huber_cost, n_downweighted=o.n_downweighted)


def _rig_host_cams(cameras):
    """The at_rig_host_cam array of rig_pose_host's `cameras`, its length, and the records it
    points into."""
    cameras = list(cameras)
    arr = (AtRigHostCam * max(1, len(cameras)))()
    keep = []
    ext, _n = _rig_extrinsics([c[3] for c in cameras], len(cameras))
    for i, (dets, poses, cam, _e) in enumerate(cameras):
        if len(dets) != len(poses):
            raise ValueError("one pose per detection")
        darr, n = _detection_records(dets)
        parr = (AtPose * max(1, n))()
        for k, p in enumerate(poses):
            parr[k].id = int(p.id)
            parr[k].R[:] = [float(x) for x in np.asarray(p.R, np.float64).reshape(9)]
            parr[k].t[:] = [float(x) for x in np.asarray(p.t, np.float64).reshape(3)]
            parr[k].err = float(p.err)
        c = AtCamera(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
        keep.append((darr, parr, c))
        arr[i].dets, arr[i].poses, arr[i].n = darr, parr, n
        arr[i].cam = C.pointer(c)
        arr[i].extr = ext[i]
    return arr, len(cameras), keep


def rig_pose_host(cameras, tags, max_hamming=0, tag_size=TAG_SIZE):
    """at_rig_pose_host: the rig pose of one instant on the CPU -- the reference RigSolver.solve is
    held to.  `cameras` is one (detections, poses, camera_matrix, extrinsics) per camera: the
    frame's detections() and poses() (same order), its CameraMatrix and its (R, t) with
    x_robot = R x_cam + t (None: identity).  Raises FieldPoseError for arguments the library
    refuses."""
    L = load_library()
    arr, n, _keep = _rig_host_cams(cameras)
    tarr, nt = _field_tags(tags)
    out = AtRigPose()
    rc = L.at_rig_pose_host(arr, n, tarr, nt, int(max_hamming), float(tag_size), C.byref(out))
    if rc < 0:
        raise FieldPoseError("at_rig_pose_host", rc)
    return _rig_pose(out)


def rig_pose_robust_host(cameras, tags, cfg, max_hamming=0, tag_size=TAG_SIZE, raw=False):
    """at_rig_pose_robust_host: the robust rig pose of one instant on the CPU -- the reference
    RigSolver.solve_robust is held to.  `cameras` and `tags` as rig_pose_host, `cfg` a RigRobust.
    Returns (RigPose, RigRobustInfo); with raw=True also the two records' bytes."""
    L = load_library()
    arr, n, _keep = _rig_host_cams(cameras)
    tarr, nt = _field_tags(tags)
    out, info = AtRigPose(), AtRigRobustInfo()
    c = _rig_robust_config(cfg)
    rc = L.at_rig_pose_robust_host(arr, n, tarr, nt, int(max_hamming), float(tag_size),
                                   C.byref(c) if c is not None else None, C.byref(out), C.byref(info))
    if rc < 0:
        raise FieldPoseError("at_rig_pose_robust_host", rc)
    pose = _rig_pose(out)
    res = (pose, _rig_robust_info(info, pose))
    return res + (bytes(out), bytes(info)) if raw else res


class RigSolver:
    """at_rig: one robot pose per instant from the layout tags of every member detector (one per
    camera, all of this process and one device).  `extrinsics` is one (R, t) per detector with
    x_robot = R x_cam + t (None: identity), `layout` the (id, R, t) triples set_field_layout takes.
    The detectors must stay open while the solver is."""

    def __init__(self, detectors, extrinsics, layout, max_hamming=0):
        L = load_library()
        self.detectors = list(detectors)
        n = len(self.detectors)
        if extrinsics is not None and len(list(extrinsics)) != n:
            raise ValueError("one extrinsics pair per detector")
        hs = (C.c_void_p * max(1, n))(*[getattr(d, "_h", None) for d in self.detectors])
        ext, _n = _rig_extrinsics(extrinsics, n)
        tarr, nt = _field_tags(layout)
        h = C.c_void_p()
        self._h = None
        rc = L.at_rig_create(hs, ext, n, tarr, nt, int(max_hamming), C.byref(h))
        if rc < 0:
            raise FieldPoseError("at_rig_create", rc)
        self._h = h
        self._cap = max(d.max_batch for d in self.detectors)
        self._buf = (AtRigPose * self._cap)()

    def solve(self, cap=None):
        """at_rig_solve: one RigPose per instant of the members' last batches (pending or
        collected; the members are not collected)."""
        cap = self._cap if cap is None else min(int(cap), self._cap)
        rc = load_library().at_rig_solve(self._h, self._buf, cap)
        if rc < 0:
            raise FieldPoseError("at_rig_solve", rc)
        self.instants = rc
        return [_rig_pose(b) for b in self._buf[:min(rc, cap)]]

    def stats(self):
        """at_rig_stats of the last solve."""
        buf = (C.c_uint64 * 5)()
        n = _check(load_library().at_rig_stats(self._h, buf, len(buf)), "at_rig_stats")
        names = ("instants_solved", "tags_used", "dropped", "rejected_steps", "kernel_ns")
        return {k: int(v) for k, v in zip(names[:n], buf)}

    def solve_robust(self, cfg, cap=None, raw=False):
        """at_rig_solve_robust: one (RigPose, RigRobustInfo) per instant of the members' last batches,
        `cfg` a RigRobust.  solve() and stats() are not touched by it.  With raw=True each pair is
        followed by the two records' bytes."""
        cap = self._cap if cap is None else min(int(cap), self._cap)
        if getattr(self, "_xbuf", None) is None:
            self._xbuf = ((AtRigPose * self._cap)(), (AtRigRobustInfo * self._cap)())
        c = _rig_robust_config(cfg)
        rc = load_library().at_rig_solve_robust(self._h, C.byref(c) if c is not None else None, self._xbuf[0],
                                                self._xbuf[1], cap)
        if rc < 0:
            raise FieldPoseError("at_rig_solve_robust", rc)
        self.instants = rc
        out = []
        for f in range(min(rc, cap)):
            pose = _rig_pose(self._xbuf[0][f])
            one = (pose, _rig_robust_info(self._xbuf[1][f], pose))
            out.append(one + (bytes(self._xbuf[0][f]), bytes(self._xbuf[1][f])) if raw else one)
        return out

    def robust_stats(self):
        """at_rig_robust_stats of the last solve_robust."""
        buf = (C.c_uint64 * 5)()
        n = _check(load_library().at_rig_robust_stats(self._h, buf, len(buf)), "at_rig_robust_stats")
        names = ("instants_solved", "tags_dropped", "rounds", "starved", "kernel_ns")
        return {k: int(v) for k, v in zip(names[:n], buf)}

    def close(self):
        if getattr(self, "_h", None):
            load_library().at_rig_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


# ---- rig calibration (k_cal_*) --------------------------------------------------
def _pose_records(poses, n):
    parr = (AtPose * max(1, n))()
    for k, p in enumerate(poses):
        parr[k].id = int(p.id)
        parr[k].R[:] = [float(x) for x in np.asarray(p.R, np.float64).reshape(9)]
        parr[k].t[:] = [float(x) for x in np.asarray(p.t, np.float64).reshape(3)]
        parr[k].err = float(p.err)
    return parr


class RigCalibrator:
    """at_rigcal: the cameras' extrinsics from recorded instants.  `cameras` is one
    (camera_matrix, (R, t), free_rot, free_trans) per camera -- its CameraMatrix, its initial
    extrinsics x_robot = R x_cam + t (None: identity) and which of the two are to be solved for;
    at least one camera must have both held fixed.  `layout` is the (id, R, t) triples
    set_field_layout takes.  Raises FieldPoseError for arguments the library refuses."""

    def __init__(self, cameras, layout, max_hamming=0, tag_size=TAG_SIZE):
        L = load_library()
        cameras = list(cameras)
        self.n_cams = n = len(cameras)
        arr = (AtRigcalCamera * max(1, n))()
        ext, _n = _rig_extrinsics([c[1] for c in cameras], n)
        for i, (cam, _e, free_rot, free_trans) in enumerate(cameras):
            arr[i].cam = AtCamera(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
            arr[i].extr = ext[i]
            arr[i].free_rot, arr[i].free_trans = int(bool(free_rot)), int(bool(free_trans))
        tarr, nt = _field_tags(layout)
        h = C.c_void_p()
        self._h = None
        rc = L.at_rigcal_create(arr, n, tarr, nt, int(max_hamming), float(tag_size), C.byref(h))
        if rc < 0:
            raise FieldPoseError("at_rigcal_create", rc)
        self._h = h

    def add(self, per_camera_results):
        """at_rigcal_add: one instant, per camera (detections, poses) of its frame in the same
        order (None or empty: the camera saw nothing).  True if the instant was stored, False if
        fewer than two cameras had a layout tag.  FieldPoseError (AT_E_CAPACITY) beyond
        AT_RIGCAL_MAX_INSTANTS."""
        arr, _keep = self._frames(per_camera_results)
        rc = load_library().at_rigcal_add(self._h, arr)
        if rc < 0:
            raise FieldPoseError("at_rigcal_add", rc)
        return bool(rc)

    def _frames(self, per_camera_results):
        """The at_rigcal_frame array of one instant, and the records it points into."""
        per = list(per_camera_results)
        if len(per) != self.n_cams:
            raise ValueError("one (detections, poses) pair per camera")
        arr = (AtRigcalFrame * self.n_cams)()
        keep = []
        for i, r in enumerate(per):
            dets, poses = r if r is not None else ((), ())
            dets, poses = list(dets), list(poses)
            if len(dets) != len(poses):
                raise ValueError("one pose per detection")
            darr, n = _detection_records(dets)
            parr = _pose_records(poses, n)
            keep.append((darr, parr))
            arr[i].dets, arr[i].poses, arr[i].n = darr, parr, n
        return arr, keep

    def __len__(self):
        return int(load_library().at_rigcal_count(self._h))

    def clear(self):
        _check(load_library().at_rigcal_clear(self._h), "at_rigcal_clear")

    def _solve(self, name):
        out = AtRigcalResult()
        rc = getattr(load_library(), name)(self._h, C.byref(out))
        if rc < 0:
            raise FieldPoseError(name, rc)
        self.record = out
        n = out.n_cams
        return RigCalibration(R=[np.array(list(out.cams[i].R)).reshape(3, 3) for i in range(n)],
                              t=[np.array(list(out.cams[i].t)) for i in range(n)],
                              cov=[np.array(list(out.cams[i].cov)).reshape(6, 6) for i in range(n)],
                              cov_valid=bool(out.cov_valid), rms_before=out.rms_before, rms_after=out.rms_after,
                              instants_used=out.instants_used, instants_skipped=out.instants_skipped,
                              accepted=out.accepted, rejected=out.rejected)

    def solve(self):
        """at_rigcal_solve: the solve on the GPU (the current device), on the calibrator's own stream."""
        return self._solve("at_rigcal_solve")

    def solve_host(self):
        """at_rigcal_solve_host: the same solve on the CPU, bit-equal records."""
        return self._solve("at_rigcal_solve_host")

    def instants(self):
        """at_rigcal_instants: one RigCalInstant per stored instant of the last solve."""
        L = load_library()
        n = _check(L.at_rigcal_instants(self._h, None, 0), "at_rigcal_instants")
        buf = (AtRigcalInstant * max(1, n))()
        n = _check(L.at_rigcal_instants(self._h, buf, n), "at_rigcal_instants")
        return [RigCalInstant(R=np.array(list(b.R)).reshape(3, 3), t=np.array(list(b.t)), rms_px=b.rms_px,
                              n_tags=b.n_tags, used=bool(b.used)) for b in buf[:n]]

    def set_profiling(self, on=True):
        _check(load_library().at_rigcal_set_profiling(self._h, int(bool(on))), "at_rigcal_set_profiling")

    def stats(self):
        """at_rigcal_stats of the last solve."""
        buf = (C.c_uint64 * 5)()
        n = _check(load_library().at_rigcal_stats(self._h, buf, len(buf)), "at_rigcal_stats")
        names = ("instants_used", "instants_skipped", "accepted_steps", "rejected_steps", "kernel_ns")
        return {k: int(v) for k, v in zip(names[:n], buf)}

    def close(self):
        if getattr(self, "_h", None):
            load_library().at_rigcal_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


# ---- rig track (k_trk_*) -----------------------------------------------------------
class RigTracker:
    """at_rigtrack: the robot's pose over a sliding window of instants linked by odometry (a
    fixed-lag smoother).  `cameras` is one (camera_matrix, (R, t)) per camera -- its CameraMatrix and
    its extrinsics x_robot = R x_cam + t (None: identity); `layout` the (id, R, t) triples
    set_field_layout takes; `sigma_px` the standard deviation of a corner in pixels; `window` the
    instants kept (2..64), `iters` the Levenberg-Marquardt iterations of a solve (1..16).  Raises
    FieldPoseError for arguments the library refuses."""

    def __init__(self, cameras, layout, max_hamming=0, tag_size=TAG_SIZE, sigma_px=0.5, window=32, iters=6):
        L = load_library()
        cameras = list(cameras)
        self.n_cams = n = len(cameras)
        arr = (AtRigtrackCamera * max(1, n))()
        ext, _n = _rig_extrinsics([c[1] for c in cameras], n)
        for i, (cam, _e) in enumerate(cameras):
            arr[i].cam = AtCamera(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
            arr[i].extr = ext[i]
        tarr, nt = _field_tags(layout)
        h = C.c_void_p()
        self._h = None
        rc = L.at_rigtrack_create(arr, n, tarr, nt, int(max_hamming), float(tag_size), float(sigma_px), int(window),
                                  int(iters), C.byref(h))
        if rc < 0:
            raise FieldPoseError("at_rigtrack_create", rc)
        self._h = h

    _frames = RigCalibrator._frames

    def push(self, per_camera_results, odometry=None, stamp=0.0):
        """at_rigtrack_push: one instant, per camera (detections, poses) of its frame (None or empty:
        the camera saw nothing; an instant without any tag is stored too).  `odometry` is
        (R, t, sigma_rot, sigma_trans): the robot now in the previous instant's robot frame,
        x_prev = R x_now + t; None starts a new chain (the window is emptied first).  Returns the
        window's count."""
        arr, _keep = self._frames(per_camera_results)
        od = None
        if odometry is not None:
            R, t, sigma_rot, sigma_trans = odometry
            od = AtRigtrackOdom(sigma_rot=float(sigma_rot), sigma_trans=float(sigma_trans))
            od.R[:] = [float(x) for x in np.asarray(R, np.float64).reshape(9)]
            od.t[:] = [float(x) for x in np.asarray(t, np.float64).reshape(3)]
        rc = load_library().at_rigtrack_push(self._h, float(stamp), arr, C.byref(od) if od is not None else None)
        if rc < 0:
            raise FieldPoseError("at_rigtrack_push", rc)
        return int(rc)

    def __len__(self):
        return int(load_library().at_rigtrack_count(self._h))

    def clear(self):
        _check(load_library().at_rigtrack_clear(self._h), "at_rigtrack_clear")

    def _solve(self, name):
        out = AtRigtrackResult()
        rc = getattr(load_library(), name)(self._h, C.byref(out))
        if rc < 0:
            raise FieldPoseError(name, rc)
        self.record = out
        return RigTrack(R=np.array(list(out.R)).reshape(3, 3), t=np.array(list(out.t)),
                        cov=np.array(list(out.cov)).reshape(6, 6), cov_valid=bool(out.cov_valid), stamp=out.stamp,
                        n=out.n, with_tags=out.with_tags, accepted=out.accepted, rejected=out.rejected,
                        cost_before=out.cost_before, cost_after=out.cost_after, rms_before=out.rms_before,
                        rms_after=out.rms_after)

    def solve(self):
        """at_rigtrack_solve: the solve on the GPU (the current device), on the tracker's own stream."""
        return self._solve("at_rigtrack_solve")

    def solve_host(self):
        """at_rigtrack_solve_host: the same solve on the CPU, bit-equal records."""
        return self._solve("at_rigtrack_solve_host")

    def instants(self):
        """at_rigtrack_instants: one RigTrackInstant per instant of the last solve, oldest first."""
        L = load_library()
        n = _check(L.at_rigtrack_instants(self._h, None, 0), "at_rigtrack_instants")
        buf = (AtRigtrackInstant * max(1, n))()
        n = _check(L.at_rigtrack_instants(self._h, buf, n), "at_rigtrack_instants")
        return [RigTrackInstant(R=np.array(list(b.R)).reshape(3, 3), t=np.array(list(b.t)), stamp=b.stamp,
                                rms_px=b.rms_px, n_tags=b.n_tags) for b in buf[:n]]

    def instant_records(self):
        """The at_rigtrack_instant records of the last solve as bytes (for equality checks)."""
        L = load_library()
        n = _check(L.at_rigtrack_instants(self._h, None, 0), "at_rigtrack_instants")
        buf = (AtRigtrackInstant * max(1, n))()
        n = _check(L.at_rigtrack_instants(self._h, buf, n), "at_rigtrack_instants")
        return bytes(buf)[:n * C.sizeof(AtRigtrackInstant)]

    def set_profiling(self, on=True):
        _check(load_library().at_rigtrack_set_profiling(self._h, int(bool(on))), "at_rigtrack_set_profiling")

    def stats(self):
        """at_rigtrack_stats of the last solve."""
        buf = (C.c_uint64 * 8)()
        n = _check(load_library().at_rigtrack_stats(self._h, buf, len(buf)), "at_rigtrack_stats")
        names = ("window", "tags_used", "accepted_steps", "rejected_steps", "kernel_ns", "start_ns", "accum_ns",
                 "solve_ns")
        return {k: int(v) for k, v in zip(names[:n], buf)}

    def close(self):
        if getattr(self, "_h", None):
            load_library().at_rigtrack_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


# ---- camera calibration (k_cc_*) ------------------------------------------------
class CameraCalibrator:
    """at_camcal: one camera's intrinsics and distortion from views of a board of tags.  `board` is
    the (id, R, t) triples set_field_layout takes, each tag's pose in the board frame; `free` the
    mask of AT_CAMCAL_* bits to solve for (0: only the view poses, which scores `init`); `init` the
    nine starting values (fx, fy, cx, cy, k1, k2, p1, p2, k3) or a (CameraMatrix, DistCoeffs) pair --
    None: the focal lengths are guessed from the tags' homographies, the principal point starts at
    the frame's centre and the distortion at zero.  Feed it detections made with zero distortion.
    Raises FieldPoseError for arguments the library refuses."""

    def __init__(self, width, height, board, tag_size=TAG_SIZE, free=AT_CAMCAL_ALL, init=None, max_hamming=0):
        L = load_library()
        cfg = AtCamcalConfig(width=int(width), height=int(height), free_mask=int(free), guess=int(init is None))
        if init is not None:
            if len(init) == 2:
                cm, dc = init
                init = (cm.fx, cm.fy, cm.cx, cm.cy, dc.k1, dc.k2, dc.p1, dc.p2, dc.k3)
            vals = [float(x) for x in init]
            if len(vals) != 9:
                raise ValueError("init holds fx, fy, cx, cy, k1, k2, p1, p2, k3")
            cfg.init = AtCamera(*vals)
        tarr, nt = _field_tags(board)
        h = C.c_void_p()
        self._h = None
        rc = L.at_camcal_create(C.byref(cfg), tarr, nt, int(max_hamming), float(tag_size), C.byref(h))
        if rc < 0:
            raise FieldPoseError("at_camcal_create", rc)
        self._h = h

    def add(self, dets):
        """at_camcal_add: one frame's detections.  True if a board tag was stored, False if the frame
        had none.  FieldPoseError (AT_E_CAPACITY) beyond AT_CAMCAL_MAX_VIEWS."""
        arr, n = _detection_records(dets)
        rc = load_library().at_camcal_add(self._h, arr, n)
        if rc < 0:
            raise FieldPoseError("at_camcal_add", rc)
        return bool(rc)

    def __len__(self):
        return int(load_library().at_camcal_count(self._h))

    def clear(self):
        _check(load_library().at_camcal_clear(self._h), "at_camcal_clear")

    def _solve(self, name):
        out = AtCamcalResult()
        rc = getattr(load_library(), name)(self._h, C.byref(out))
        if rc < 0:
            raise FieldPoseError(name, rc)
        self.record = out
        return CameraCalibration(params=np.array([getattr(out.cam, k) for k in CAMCAL_PARAMS]),
                                 cov=np.array(list(out.cov)).reshape(9, 9), cov_valid=bool(out.cov_valid),
                                 rms_before=out.rms_before, rms_after=out.rms_after, views_used=out.views_used,
                                 views_skipped=out.views_skipped, corners=out.corners, accepted=out.accepted,
                                 rejected=out.rejected)

    def solve(self):
        """at_camcal_solve: the solve on the GPU (the current device), on the calibrator's own stream."""
        return self._solve("at_camcal_solve")

    def solve_host(self):
        """at_camcal_solve_host: the same solve on the CPU, bit-equal records."""
        return self._solve("at_camcal_solve_host")

    def views(self):
        """at_camcal_views: one CameraCalView per stored view of the last solve."""
        L = load_library()
        n = _check(L.at_camcal_views(self._h, None, 0), "at_camcal_views")
        buf = (AtCamcalView * max(1, n))()
        n = _check(L.at_camcal_views(self._h, buf, n), "at_camcal_views")
        return [CameraCalView(R=np.array(list(b.R)).reshape(3, 3), t=np.array(list(b.t)), rms_px=b.rms_px,
                              n_tags=b.n_tags, used=bool(b.used)) for b in buf[:n]]

    def set_profiling(self, on=True):
        _check(load_library().at_camcal_set_profiling(self._h, int(bool(on))), "at_camcal_set_profiling")

    def stats(self):
        """at_camcal_stats of the last solve."""
        buf = (C.c_uint64 * 5)()
        n = _check(load_library().at_camcal_stats(self._h, buf, len(buf)), "at_camcal_stats")
        names = ("views_used", "views_skipped", "accepted_steps", "rejected_steps", "kernel_ns")
        return {k: int(v) for k, v in zip(names[:n], buf)}

    def close(self):
        if getattr(self, "_h", None):
            load_library().at_camcal_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


# ---- field map (k_fm_*) -----------------------------------------------------------
class FieldMapper:
    """at_fieldmap: where the tags of a field stand, from recorded views.  `tags` is one
    (id, R, t, free_rot, free_trans) per map tag -- its start x_field = R x_tag + t and which of the
    two are to be solved for; R = None marks a tag without a start (known = 0), which is placed from
    views that see it together with placed tags.  At least one tag must have a start and both flags
    false: the anchor.  Raises FieldPoseError for arguments the library refuses."""

    def __init__(self, tags, max_hamming=0, tag_size=TAG_SIZE):
        L = load_library()
        tags = list(tags)
        n = len(tags)
        arr = (AtFieldmapTag * max(1, n))()
        for i, (tid, R, t, free_rot, free_trans) in enumerate(tags):
            arr[i].tag.id = int(tid)
            arr[i].known = int(R is not None)
            if R is not None:
                arr[i].tag.R[:] = [float(x) for x in np.asarray(R, np.float64).reshape(9)]
                arr[i].tag.t[:] = [float(x) for x in np.asarray(t, np.float64).reshape(3)]
            arr[i].free_rot, arr[i].free_trans = int(bool(free_rot)), int(bool(free_trans))
        h = C.c_void_p()
        self._h = None
        rc = L.at_fieldmap_create(arr, n, int(max_hamming), float(tag_size), C.byref(h))
        if rc < 0:
            raise FieldPoseError("at_fieldmap_create", rc)
        self._h = h

    def add(self, dets, poses, camera_matrix=None):
        """at_fieldmap_add: one frame's detections and poses (same order) and its camera's
        CameraMatrix.  True if the view was stored, False if fewer than two map tags were in it.
        FieldPoseError (AT_E_CAPACITY) beyond AT_FIELDMAP_MAX_VIEWS."""
        dets, poses = list(dets), list(poses)
        if len(dets) != len(poses):
            raise ValueError("one pose per detection")
        cam = camera_matrix or TEST_CAMERA
        darr, n = _detection_records(dets)
        parr = _pose_records(poses, n)
        c = AtCamera(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)
        rc = load_library().at_fieldmap_add(self._h, darr, parr, n, C.byref(c))
        if rc < 0:
            raise FieldPoseError("at_fieldmap_add", rc)
        return bool(rc)

    def __len__(self):
        return int(load_library().at_fieldmap_count(self._h))

    def clear(self):
        _check(load_library().at_fieldmap_clear(self._h), "at_fieldmap_clear")

    def _solve(self, name):
        out = AtFieldmapResult()
        rc = getattr(load_library(), name)(self._h, C.byref(out))
        if rc < 0:
            raise FieldPoseError(name, rc)
        self.record = out
        return FieldMap(rms_before=out.rms_before, rms_after=out.rms_after, views_used=out.views_used,
                        views_skipped=out.views_skipped, corners=out.corners, accepted=out.accepted,
                        rejected=out.rejected, cov_valid=bool(out.cov_valid), n_tags=out.n_tags,
                        n_placed=out.n_placed)

    def solve(self):
        """at_fieldmap_solve: the solve on the GPU (the current device), on the mapper's own stream."""
        return self._solve("at_fieldmap_solve")

    def solve_host(self):
        """at_fieldmap_solve_host: the same solve on the CPU, bit-equal records."""
        return self._solve("at_fieldmap_solve_host")

    def tag_records(self):
        """The at_fieldmap_tag_result array of the last solve (the bit-exact view) and its length."""
        L = load_library()
        n = _check(L.at_fieldmap_tags(self._h, None, 0), "at_fieldmap_tags")
        buf = (AtFieldmapTagResult * max(1, n))()
        return buf, _check(L.at_fieldmap_tags(self._h, buf, n), "at_fieldmap_tags")

    def tags(self):
        """at_fieldmap_tags: one FieldMapTag per map tag of the last solve, in the order given."""
        buf, n = self.tag_records()
        return [FieldMapTag(id=b.id, placed=bool(b.placed), R=np.array(list(b.R)).reshape(3, 3), t=np.array(list(b.t)),
                            R0=np.array(list(b.R0)).reshape(3, 3), t0=np.array(list(b.t0)),
                            cov=np.array(list(b.cov)).reshape(6, 6), views=b.views) for b in buf[:n]]

    def view_records(self):
        """The at_fieldmap_view array of the last solve and its length."""
        L = load_library()
        n = _check(L.at_fieldmap_views(self._h, None, 0), "at_fieldmap_views")
        buf = (AtFieldmapView * max(1, n))()
        return buf, _check(L.at_fieldmap_views(self._h, buf, n), "at_fieldmap_views")

    def views(self):
        """at_fieldmap_views: one FieldMapView per stored view of the last solve."""
        buf, n = self.view_records()
        return [FieldMapView(R=np.array(list(b.R)).reshape(3, 3), t=np.array(list(b.t)), rms_px=b.rms_px,
                             n_tags=b.n_tags, used=bool(b.used)) for b in buf[:n]]

    def set_profiling(self, on=True):
        _check(load_library().at_fieldmap_set_profiling(self._h, int(bool(on))), "at_fieldmap_set_profiling")

    def stats(self):
        """at_fieldmap_stats of the last solve."""
        buf = (C.c_uint64 * 6)()
        n = _check(load_library().at_fieldmap_stats(self._h, buf, len(buf)), "at_fieldmap_stats")
        names = ("views_used", "views_skipped", "accepted_steps", "rejected_steps", "kernel_ns", "dropped")
        return {k: int(v) for k, v in zip(names[:n], buf)}

    def close(self):
        if getattr(self, "_h", None):
            load_library().at_fieldmap_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def _check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed: %s (%d)" % (what, load_library().at_strerror(rc).decode(), rc))
    return rc


class GpuDetector:
    """Drop-in for frc971::apriltag::GpuDetector on MI355X (one instance per camera)."""

    MAX_DETECTIONS = 64  # per frame in the collect buffer; frames with more are fetched whole (at_detections)
    DEBUG_TAPS = False     # default of debug_taps (the parity tests turn it on for their module)

    def __init__(self, width, height, camera_matrix: CameraMatrix = TEST_CAMERA,
                 distortion_coefficients: DistCoeffs = TEST_DIST, family="tag36h11",
                 max_batch=1, device=0, pinned_out=False, debug_taps=None, **overrides):
        L = load_library()
        self.width, self.height, self.max_batch = int(width), int(height), int(max_batch)
        cfg = AtConfig()
        L.at_config_default(C.byref(cfg), self.width, self.height)
        self._family = family.encode()
        cfg.family = self._family
        cfg.max_batch = self.max_batch
        cfg.device = int(device)
        for k, v in overrides.items():
            setattr(cfg, k, v)
        cam = AtCamera(fx=camera_matrix.fx, fy=camera_matrix.fy, cx=camera_matrix.cx, cy=camera_matrix.cy,
                       k1=distortion_coefficients.k1, k2=distortion_coefficients.k2,
                       p1=distortion_coefficients.p1, p2=distortion_coefficients.p2,
                       k3=distortion_coefficients.k3)
        h = C.c_void_p()
        _check(L.at_create(C.byref(cfg), C.byref(cam), C.byref(h)), "at_create")
        self._h = h
        if self.DEBUG_TAPS if debug_taps is None else debug_taps:
            _check(L.at_set_debug_taps(h, 1), "at_set_debug_taps")  # copy_blob_points needs them
        self._cap = self.MAX_DETECTIONS
        self._out_t = None
        if pinned_out:
            # at_collect writes the detections straight into page-locked memory (torch owns
            # it), so a caller can copy them to the device asynchronously without staging
            import torch
            nb = C.sizeof(AtDetection) * self._cap * self.max_batch
            self._out_t = torch.empty(nb, dtype=torch.uint8).pin_memory()
            self._out = (AtDetection * (self._cap * self.max_batch)).from_address(self._out_t.data_ptr())
        else:
            self._out = (AtDetection * (self._cap * self.max_batch))()
        self._n = (C.c_int * self.max_batch)()
        self._last = [[] for _ in range(self.max_batch)]
        self._last_status = 0
        self._mjpg_device_entropy = False
        self.undistort = False

    def close(self):
        if getattr(self, "_h", None):
            load_library().at_destroy(self._h)
            self._h = None
        if getattr(self, "_jpeg_buf", None) is not None:
            load_library().at_host_free(self._jpeg_buf)
            self._jpeg_buf = None

    def __del__(self):
        self.close()

    # ---- detection ---------------------------------------------------------
    def _frame_records(self, f):
        """at_detection records of frame f of the last batch (all of them: a frame with
        more than the collect buffer holds is fetched again with at_detections)."""
        n = self._n[f]
        if n <= self._cap:
            return [self._out[f * self._cap + i] for i in range(n)]
        buf = (AtDetection * n)()
        got = _check(load_library().at_detections(self._h, f, buf, n), "at_detections")
        return list(buf[:got])

    def frame_record_bytes(self, f):
        """Every at_detection record of frame f of the last batch, as bytes (what a peer
        sends rank 0, multigpu.RecordGather)."""
        return b"".join(bytes(r) for r in self._frame_records(f))

    def _unpack(self, nframes):
        res = []
        for f in range(nframes):
            dets = []
            for d in self._frame_records(f):
                dets.append(Detection(id=d.id, hamming=d.hamming, decision_margin=d.decision_margin,
                                      H=np.array(list(d.H)).reshape(3, 3), c=np.array(list(d.c)),
                                      p=np.array([[d.p[k][0], d.p[k][1]] for k in range(4)])))
            res.append(dets)
        self._last = res
        return res

    def detect(self, frame: np.ndarray, fmt: int = AT_FMT_YUYV):
        """GpuDetector::Detect (apriltag_gpu.cu:725): one host frame, synchronous."""
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        rc = load_library().at_detect(self._h, frame.ctypes.data, fmt, self._out, self._cap, self._n)
        self._last_status = rc
        if rc < 0 and rc != AT_E_CAPACITY:
            _check(rc, "at_detect")
        return self._unpack(1)[0]

    def detect_count(self, frame: np.ndarray, fmt: int = AT_FMT_YUYV):
        """at_detect without building Python objects: returns the detection count
        (the detections are in this detector's at_detection buffer)."""
        rc = load_library().at_detect(self._h, frame.ctypes.data, fmt, self._out, self._cap, self._n)
        if rc < 0 and rc != AT_E_CAPACITY:
            _check(rc, "at_detect")
        return self._n[0]

    def detect_batch(self, frames, fmt: int = AT_FMT_YUYV):
        frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        rc = load_library().at_detect_batch(self._h, ptrs, len(frames), fmt, self._out, self._cap, self._n)
        self._last_status = rc
        if rc < 0 and rc != AT_E_CAPACITY:
            _check(rc, "at_detect_batch")
        return self._unpack(len(frames))

    def detect_device(self, dev_ptr: int, frame_stride: int, nframes: int, fmt: int = AT_FMT_YUYV,
                      counts_only=False):
        """Frames already resident in device memory (e.g. a torch.cuda tensor's data_ptr())."""
        rc = load_library().at_detect_device(self._h, C.c_void_p(dev_ptr), frame_stride, nframes, fmt,
                                             self._out, self._cap, self._n)
        self._last_status = rc
        if rc < 0 and rc != AT_E_CAPACITY:
            _check(rc, "at_detect_device")
        if counts_only:
            return [self._n[f] for f in range(nframes)]
        return self._unpack(nframes)

    def enqueue_device(self, dev_ptr: int, frame_stride: int, nframes: int, fmt: int = AT_FMT_YUYV):
        _check(load_library().at_enqueue_device(self._h, C.c_void_p(dev_ptr), frame_stride, nframes, fmt),
               "at_enqueue_device")
        self._pending = nframes

    def enqueue_host(self, host_ptrs, fmt: int = AT_FMT_YUYV):
        """at_enqueue_host: host frames (addresses; page-locked for an asynchronous
        copy) copied and detected on this detector's stream; collect() later."""
        ptrs = (C.c_void_p * len(host_ptrs))(*host_ptrs)
        _check(load_library().at_enqueue_host(self._h, ptrs, len(host_ptrs), fmt), "at_enqueue_host")
        self._pending = len(host_ptrs)

    # ---- MJPG camera frames (host entropy decode, k_mjpg_idct on the GPU) ------
    def _mjpg_args(self, jpgs):
        jpgs = [bytes(j) for j in jpgs]
        ptrs = (C.c_char_p * len(jpgs))(*jpgs)
        lens = (C.c_size_t * len(jpgs))(*[len(j) for j in jpgs])
        return jpgs, ptrs, lens

    def enqueue_mjpg(self, jpgs):
        """at_enqueue_mjpg: a batch of JPEG frames (bytes); collect() later.  A frame the
        library refuses raises MjpgError (its index and code) and enqueues nothing."""
        _keep, ptrs, lens = self._mjpg_args(jpgs)
        bad = C.c_int(-1)
        rc = load_library().at_enqueue_mjpg(self._h, ptrs, lens, len(jpgs), C.byref(bad))
        if rc in (AT_E_UNSUPPORTED, AT_E_INVALID):
            raise MjpgError("at_enqueue_mjpg", rc, bad.value if bad.value >= 0 else None)
        _check(rc, "at_enqueue_mjpg")
        self._pending = len(jpgs)

    def detect_mjpg_batch(self, jpgs):
        """at_detect_mjpg_batch: JPEG frames in, detections per frame out (synchronous)."""
        _keep, ptrs, lens = self._mjpg_args(jpgs)
        bad = C.c_int(-1)
        rc = load_library().at_detect_mjpg_batch(self._h, ptrs, lens, len(jpgs), self._out, self._cap, self._n,
                                                 C.byref(bad))
        self._last_status = rc
        if rc == AT_E_INVALID and bad.value < 0 and self._mjpg_device_entropy:
            # bad entropy-coded data, seen on the device: those frames are empty (frame_status
            # tells which), the others' results are valid
            return self._unpack(len(jpgs))
        if rc in (AT_E_UNSUPPORTED, AT_E_INVALID):
            raise MjpgError("at_detect_mjpg_batch", rc, bad.value if bad.value >= 0 else None)
        if rc < 0 and rc != AT_E_CAPACITY:
            _check(rc, "at_detect_mjpg_batch")
        return self._unpack(len(jpgs))

    def detect_mjpg(self, jpg: bytes):
        """at_detect_mjpg: one JPEG frame, synchronous."""
        return self.detect_mjpg_batch([jpg])[0]

    def set_mjpg_threads(self, n: int):
        """Host threads decoding the frames of one MJPG batch (1..16, default 1)."""
        _check(load_library().at_mjpg_set_threads(self._h, int(n)), "at_mjpg_set_threads")

    def set_mjpg_color(self, on=True):
        """at_mjpg_set_color: from the next MJPG batch on, also decode chroma and produce each
        frame's BGR8 image on the GPU (copy_bgr, mjpg_bgr_ptr, annotate_staged, the
        game-piece tensors).  Off by default."""
        _check(load_library().at_mjpg_set_color(self._h, int(bool(on))), "at_mjpg_set_color")

    def set_mjpg_device_entropy(self, on=True):
        """at_mjpg_set_device_entropy: from the next MJPG batch on the host only parses the
        markers and the GPU decodes the entropy-coded data too (k_mjpg_entropy).  A frame whose
        data turns out bad there is empty, frame_status gives AT_E_INVALID for it and
        last_status is AT_E_INVALID; the other frames' results stand.  Off by default."""
        _check(load_library().at_mjpg_set_device_entropy(self._h, int(bool(on))), "at_mjpg_set_device_entropy")
        self._mjpg_device_entropy = bool(on)

    def set_mjpg_subseq(self, nbytes: int):
        """at_mjpg_set_subseq: the piece size S of the device entropy decode (16..256, a power of two)."""
        _check(load_library().at_mjpg_set_subseq(self._h, int(nbytes)), "at_mjpg_set_subseq")

    @property
    def last_status(self):
        """Code of the last synchronous detect call or collect (0, AT_E_CAPACITY, AT_E_INVALID)."""
        return self._last_status

    def mjpg_bgr_ptr(self, frame=0):
        """at_mjpg_bgr: device pointer of frame `frame`'s BGR8 image of the last (colour-on
        MJPG) batch, valid until the next batch."""
        ptr = C.c_void_p()
        _check(load_library().at_mjpg_bgr(self._h, frame, C.byref(ptr)), "at_mjpg_bgr")
        return ptr.value

    def copy_bgr(self, frame=0):
        """at_mjpg_copy_bgr: host copy (H, W, 3) uint8 of that image; raises unless the last
        batch was an MJPG batch enqueued with colour on."""
        out = np.empty((self.height, self.width, 3), np.uint8)
        _check(load_library().at_mjpg_copy_bgr(self._h, frame, out.ctypes.data, out.size), "at_mjpg_copy_bgr")
        return out

    MJPG_STATS = ("compressed_bytes", "device_bytes", "dense_frames", "host_decode_us", "idct_kernel_ns",
                  "color_kernels_ns", "entropy_kernel_ns", "host_route_frames", "sync_rounds")

    def mjpg_stats(self):
        """at_mjpg_stats of the last MJPG batch."""
        buf = (C.c_uint64 * len(self.MJPG_STATS))()
        n = _check(load_library().at_mjpg_stats(self._h, buf, len(buf)), "at_mjpg_stats")
        return dict(zip(self.MJPG_STATS, [int(x) for x in buf[:n]]))

    def wait_stream(self, stream_handle: int):
        """at_stream_wait: the next enqueued batch waits (on the GPU) for the work queued
        so far on a HIP stream, e.g. torch.cuda.current_stream().cuda_stream."""
        _check(load_library().at_stream_wait(self._h, C.c_void_p(stream_handle)), "at_stream_wait")

    def poses(self, frame=0):
        """Pose of each detection of `frame` of the last batch (same order as its
        detections), computed on the GPU (k_pose) when tag_size > 0."""
        cap = max(self._n[frame], 1)
        buf = (AtPose * cap)()
        n = _check(load_library().at_poses(self._h, frame, buf, cap), "at_poses")
        return [Pose(id=b.id, R=np.array(list(b.R)).reshape(3, 3), t=np.array(list(b.t)), err=b.err)
                for b in buf[:min(n, cap)]]

    # ---- ideal corners (the head of the pose stage) ----------------------------
    def set_undistort(self, on=True):
        """at_set_undistort: from the next batch on the tag, field and rig poses come from ideal
        corners (the lens distortion undone); detections() and the drawings stay raw."""
        _check(load_library().at_set_undistort(self._h, int(bool(on))), "at_set_undistort")
        self.undistort = bool(on)

    def ideal_detections(self, frame=0):
        """at_ideal_detections: `frame`'s detections with H, c and p ideal, same order as
        detections(frame); id = -1 where a corner is not invertible."""
        cap = max(self._n[frame], 1)
        buf = (AtDetection * cap)()
        n = _check(load_library().at_ideal_detections(self._h, frame, buf, cap), "at_ideal_detections")
        return _detections_of(buf[:min(n, cap)])

    def undistort_points(self, xy):
        """at_undistort_points: (n, 2) raw pixels -> ((n, 2) ideal pixels, (n,) bool ok) on the GPU
        (k_und_points), with this detector's lens."""
        xy, out, ok = _points_in(xy)
        dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        _check(load_library().at_undistort_points(self._h, xy.ctypes.data_as(dp), len(xy), out.ctypes.data_as(dp),
                                                  ok.ctypes.data_as(bp)), "at_undistort_points")
        return out, ok.astype(bool)

    UNDISTORT_STATS = ("ideal", "not_invertible")

    def undistort_stats(self):
        """at_undistort_stats of the last collected batch."""
        buf = (C.c_uint64 * len(self.UNDISTORT_STATS))()
        n = _check(load_library().at_undistort_stats(self._h, buf, len(buf)), "at_undistort_stats")
        return dict(zip(self.UNDISTORT_STATS, [int(x) for x in buf[:n]]))

    # ---- field pose (k_field) ------------------------------------------------
    def set_field_layout(self, tags, max_hamming=0):
        """at_set_field_layout: where each tag stands on the field -- (id, R, t) triples,
        x_field = R x_tag + t -- from the next batch on; empty or None clears it.  Raises
        FieldPoseError (AT_E_INVALID) for a bad layout, tag_size 0 or a batch not yet collected."""
        arr, n = _field_tags(tags)
        rc = load_library().at_set_field_layout(self._h, arr, n, int(max_hamming))
        if rc < 0:
            raise FieldPoseError("at_set_field_layout", rc)

    def field_poses(self):
        """at_field_poses: one FieldPose per frame of the last collected batch."""
        buf = (AtFieldPose * self.max_batch)()
        rc = load_library().at_field_poses(self._h, buf, self.max_batch)
        if rc < 0:
            raise FieldPoseError("at_field_poses", rc)
        return [_field_pose(b) for b in buf[:rc]]

    FIELD_STATS = ("frames_solved", "tags_used", "dropped_by_cap", "rejected_steps", "kernel_ns")

    def field_stats(self):
        """at_field_stats of the last collected batch."""
        buf = (C.c_uint64 * len(self.FIELD_STATS))()
        n = _check(load_library().at_field_stats(self._h, buf, len(buf)), "at_field_stats")
        return dict(zip(self.FIELD_STATS, [int(x) for x in buf[:n]]))

    def collect(self, counts_only=False):
        """at_collect: wait for the batch, run the host tail.  The detections land in
        this detector's at_detection buffer; counts_only=True skips building Python
        objects from it and returns the per-frame counts (what a C++ caller sees)."""
        rc = load_library().at_collect(self._h, self._out, self._cap, self._n)
        self._last_status = rc
        if rc < 0 and rc != AT_E_CAPACITY and not (rc == AT_E_INVALID and self._mjpg_device_entropy and self._pending):
            _check(rc, "at_collect")
        if counts_only:
            return [self._n[f] for f in range(self._pending)]
        return self._unpack(self._pending)

    def results(self):
        """Detections of every frame of the last collected batch (after
        collect(counts_only=True), builds the Python objects from the buffer)."""
        return self._unpack(self._pending)

    # ---- per-stage timing (the reference's CudaEvent stage timers,
    #      apriltag_gpu.cu:1118-1163) ----------------------------------------
    def set_profiling(self, enable=True):
        _check(load_library().at_set_profiling(self._h, int(enable)), "at_set_profiling")

    def stage_times(self):
        """{stage name: (mean ms per batch, batches)} accumulated since profiling was enabled."""
        L = load_library()
        buf = (C.c_double * 32)()
        n = _check(L.at_stage_times(self._h, buf, 32), "at_stage_times")
        batches = int(buf[n]) if n < 32 else 0
        return {L.at_stage_name(i).decode(): buf[i] for i in range(n)}, batches

    def set_kernel_timer(self, stage_name=None):
        """Time one kernel live inside the normal launch sequence (None: off)."""
        L = load_library()
        stage = -1
        if stage_name is not None:
            names = [L.at_stage_name(i).decode() for i in range(32)]
            stage = names.index(stage_name)
        _check(L.at_set_kernel_timer(self._h, stage), "at_set_kernel_timer")

    def kernel_time(self):
        """(mean ms per launch, launches) of the timed kernel (HIP events on its stream)."""
        ms, n = C.c_double(), C.c_longlong()
        _check(load_library().at_kernel_time(self._h, C.byref(ms), C.byref(n)), "at_kernel_time")
        return ms.value, n.value

    def kernel_span(self):
        """(mean ms per launch, launches) of the timed kernel on the device clock (first
        workgroup start -> last workgroup end; the span a rocprofv3 kernel trace times)."""
        ms, n = C.c_double(), C.c_longlong()
        _check(load_library().at_kernel_span(self._h, C.byref(ms), C.byref(n)), "at_kernel_span")
        return ms.value, n.value

    BATCH_STATS = ("frames", "boundary_points", "pairs", "small_blob_points", "large_blob_points",
                   "quads", "candidates", "host_wait_us_total", "host_tail_us_total", "ccl_listed_roots",
                   "ccl_listed_roots_max", "ccl_fallback_frames")

    def batch_stats(self):
        """Work counts of the last collected batch (see at_batch_stats)."""
        buf = (C.c_uint64 * len(self.BATCH_STATS))()
        n = _check(load_library().at_batch_stats(self._h, buf, len(buf)), "at_batch_stats")
        return dict(zip(self.BATCH_STATS, [int(x) for x in buf[:n]]))

    def detections(self, frame=0):
        """GpuDetector::Detections (apriltag_gpu.h:93), sorted by id."""
        return self._last[frame]

    def _records_array(self, frame):
        recs = self._frame_records(frame)
        arr = (AtDetection * max(1, len(recs)))(*recs)
        return arr, len(recs)

    def draw_outlines_device(self, bgr_ptr: int, frame=0):
        """at_draw_outlines_device: the annotated image of `frame` of the last batch
        (outlines and ids, apriltag_utils.cu:54-79) drawn onto the device-resident
        BGR8 image at `bgr_ptr` (width x height x 3)."""
        arr, n = self._records_array(frame)
        _check(load_library().at_draw_outlines_device(self._h, arr, n, bgr_ptr), "at_draw_outlines_device")

    def annotate_staged(self, frame=0):
        """at_annotate_staged: the annotated image of host BGR8 frame `frame` of the last
        batch, drawn on its staged copy in HBM (after a colour-on MJPG batch: on the
        decoded image); returns it (H, W, 3) uint8."""
        arr, n = self._records_array(frame)
        out = np.empty((self.height, self.width, 3), np.uint8)
        _check(load_library().at_annotate_staged(self._h, frame, arr, n, out.ctypes.data), "at_annotate_staged")
        return out

    # ---- the annotated image as a JPEG, encoded on the GPU -----------------------
    def _jpeg_out(self, sampling, cap):
        """(code, capacity, buffer): a page-locked buffer of the worst-case size, allocated
        once per detector (at_host_alloc: the stream's bytes arrive by DMA)."""
        s = _jpeg_sampling(sampling)
        L = load_library()
        if getattr(self, "_jpeg_buf", None) is None:
            self._jpeg_cap = max(int(L.at_jpeg_max_bytes(self.width, self.height, k)) for k in (0, 1, 2))
            if not self._jpeg_cap:
                raise JpegError("at_jpeg_max_bytes", AT_E_INVALID)
            p = C.c_void_p()
            _check(L.at_host_alloc(self._jpeg_cap, C.byref(p)), "at_host_alloc")
            self._jpeg_buf = p
        return s, (self._jpeg_cap if cap is None else min(int(cap), self._jpeg_cap))

    def _jpeg_result(self, rc, what, n):
        if rc in (AT_E_INVALID, AT_E_CAPACITY):
            raise JpegError(what, rc, n.value)
        _check(rc, what)
        return C.string_at(self._jpeg_buf, n.value)

    def encode_jpeg_device(self, bgr_ptr: int, quality=95, sampling="4:2:0", cap=None):
        """at_encode_jpeg_device: the device-resident BGR8 image at `bgr_ptr` (width x height
        x 3) as a baseline JPEG (bytes), encoded on the GPU.  `cap` limits the accepted size
        (JpegError with code AT_E_CAPACITY and `needed` beyond it)."""
        s, cap = self._jpeg_out(sampling, cap)
        n = C.c_size_t()
        rc = load_library().at_encode_jpeg_device(self._h, C.c_void_p(bgr_ptr), int(quality), s, self._jpeg_buf,
                                                  cap, C.byref(n))
        return self._jpeg_result(rc, "at_encode_jpeg_device", n)

    def annotate_jpeg(self, frame=0, quality=95, sampling="4:2:0", cap=None):
        """at_annotate_jpeg: annotate_staged's image as a baseline JPEG (bytes): drawn and
        encoded on the GPU, only the compressed bytes cross the link."""
        # (a frame index no batch can have: the library refuses it)
        arr, nd = self._records_array(frame) if 0 <= frame < self.max_batch else ((AtDetection * 1)(), 0)
        s, cap = self._jpeg_out(sampling, cap)
        n = C.c_size_t()
        rc = load_library().at_annotate_jpeg(self._h, frame, arr, nd, int(quality), s, self._jpeg_buf, cap,
                                             C.byref(n))
        return self._jpeg_result(rc, "at_annotate_jpeg", n)

    JPEG_STATS = ("bytes", "encode_kernels_ns")

    def jpeg_stats(self):
        """at_jpeg_stats of the last encode."""
        buf = (C.c_uint64 * len(self.JPEG_STATS))()
        n = _check(load_library().at_jpeg_stats(self._h, buf, len(buf)), "at_jpeg_stats")
        return dict(zip(self.JPEG_STATS, [int(x) for x in buf[:n]]))

    # ---- the preview stream: a scaled annotated image of a frame of any format ----
    def preview_size(self, scale: int):
        """(pw, ph, ox, oy) of this detector's preview at `scale` (see preview_size)."""
        return preview_size(self.width, self.height, scale)

    def _preview_records(self, frame, detections, boxes):
        if detections is None:  # the frame's own (a frame index no batch can have: the library refuses it)
            arr, nd = self._records_array(frame) if 0 <= frame < self.max_batch and frame < len(self._n) else \
                ((AtDetection * 1)(), 0)
        else:
            arr, nd = _detection_records(detections)
        return arr, nd, _box_records(boxes)

    def preview_bgr(self, frame=0, scale=4, boxes=None, detections=None):
        """at_preview_bgr: the annotated preview (ph, pw, 3) uint8 of frame `frame` of the last
        host-fed batch, whatever its format (BGR8, YUYV, GRAY8, MJPG with or without colour):
        converted and box-averaged by k_preview from the staged frame, which is only read;
        the frame's detections (or `detections`) and `boxes` are drawn at preview scale."""
        pw, ph, _, _ = self.preview_size(scale)
        arr, nd, rec = self._preview_records(frame, detections, boxes)
        out = np.empty((ph, pw, 3), np.uint8)
        rc = load_library().at_preview_bgr(self._h, frame, int(scale), C.addressof(arr), nd,
                                           rec.ctypes.data if len(rec) else None, len(rec), out.ctypes.data)
        if rc == AT_E_INVALID:
            raise JpegError("at_preview_bgr", rc)
        _check(rc, "at_preview_bgr")
        return out

    def _preview_jpeg_result(self, rc, what, n, qu):
        if rc in (AT_E_INVALID, AT_E_CAPACITY):
            e = JpegError(what, rc, n.value)
            e.quality_used = qu.value
            raise e
        _check(rc, what)
        return C.string_at(self._jpeg_buf, n.value), qu.value

    def preview_jpeg(self, frame=0, scale=4, quality=50, sampling="4:2:0", max_bytes=0, boxes=None, detections=None,
                     cap=None):
        """at_preview_jpeg: preview_bgr's image as a baseline JPEG: (bytes, quality used).
        `max_bytes` > 0 is the frame's byte budget: the quality is lowered by the bounded
        bisection of at_api.h until the stream fits (JpegError AT_E_CAPACITY, `needed` and
        `quality_used` == 1 if quality 1 does not)."""
        if not 1 <= int(scale) <= 8:
            raise JpegError("at_preview_jpeg", AT_E_INVALID)
        arr, nd, rec = self._preview_records(frame, detections, boxes)
        s, cap = self._jpeg_out(sampling, cap)
        n, qu = C.c_size_t(), C.c_int()
        rc = load_library().at_preview_jpeg(self._h, frame, int(scale), C.addressof(arr), nd,
                                            rec.ctypes.data if len(rec) else None, len(rec), int(quality), s,
                                            int(max_bytes), self._jpeg_buf, cap, C.byref(n), C.byref(qu))
        return self._preview_jpeg_result(rc, "at_preview_jpeg", n, qu)

    def preview_jpeg_device(self, dev_ptr: int, fmt: int, scale=4, quality=50, sampling="4:2:0", max_bytes=0,
                            boxes=None, detections=(), cap=None):
        """at_preview_jpeg_device: the same for one device-resident frame of the detector's
        geometry in `fmt` at `dev_ptr` (8-byte aligned), e.g. a frame of an enqueue_device
        batch; `detections` are drawn as given."""
        arr, nd = _detection_records(detections)
        rec = _box_records(boxes)
        s, cap = self._jpeg_out(sampling, cap)
        n, qu = C.c_size_t(), C.c_int()
        rc = load_library().at_preview_jpeg_device(self._h, C.c_void_p(dev_ptr), int(fmt), int(scale),
                                                   C.addressof(arr), nd, rec.ctypes.data if len(rec) else None,
                                                   len(rec), int(quality), s, int(max_bytes), self._jpeg_buf, cap,
                                                   C.byref(n), C.byref(qu))
        return self._preview_jpeg_result(rc, "at_preview_jpeg_device", n, qu)

    PREVIEW_STATS = ("bytes", "quality_used", "encodes", "width", "height", "kernels_ns")

    def preview_stats(self):
        """at_preview_stats of the last preview call."""
        buf = (C.c_uint64 * len(self.PREVIEW_STATS))()
        n = _check(load_library().at_preview_stats(self._h, buf, len(buf)), "at_preview_stats")
        return dict(zip(self.PREVIEW_STATS, [int(x) for x in buf[:n]]))

    def frame_status(self, frame=0):
        return load_library().at_frame_status(self._h, frame)

    # ---- shared game-piece preprocessing (game_piece_detection_node.cu:347-379) ----
    def enable_game_piece_input(self, width=640, height=640, channels=3):
        """Also produce preprocess_image's NCHW float tensor of every BGR8 frame
        (resize INTER_LINEAR, BGR->RGB / GRAY, x 1/255) in each later batch."""
        _check(load_library().at_gp_enable(self._h, width, height, channels), "at_gp_enable")
        self._gp = (channels, height, width)

    def game_piece_tensor_ptr(self, frame=0):
        """Device pointer of frame `frame`'s tensor of the last (BGR8) batch."""
        ptr = C.c_void_p()
        _check(load_library().at_gp_tensor(self._h, frame, C.byref(ptr)), "at_gp_tensor")
        return ptr.value

    def game_piece_tensor(self, frame=0):
        """Host copy (channels, height, width) float32 of frame `frame`'s tensor."""
        out = np.empty(self._gp, np.float32)
        _check(load_library().at_gp_copy(self._h, frame, out.ctypes.data, out.size), "at_gp_copy")
        return out

    # ---- game-piece output parse (yolo_detection.h:53-209) -------------------------
    def game_piece_parse(self, raw, conf=0.25, iou=0.45, model_size=(640, 640), producer_stream=None, strict=True,
                         records=False, cap=None):
        """at_gp_parse_device: the network's output tensors, resident in device memory, to the
        boxes in camera pixels (this detector's width x height) -- confidence threshold,
        per-class greedy NMS and scaling on the GPU; only the boxes cross the link.

        `raw` is a CUDA torch tensor [4 + C, P] or [B, 4 + C, P] (float32, each frame
        contiguous), or (ptr, nframes, C, P[, frame_stride in floats]).  The parse is ordered
        after the work queued so far on `producer_stream` (a torch stream or a hipStream_t
        handle; None: the null stream), with no host wait in between.  Returns one list of
        boxes per frame, NMS order ([GamePieceBox], or GP_BOX_DTYPE records with
        records=True; at most `cap` per frame, default all).  A frame with more than
        AT_GP_MAX_CANDIDATES candidates raises GamePieceCapacityError naming it; with
        strict=False that frame is instead computed by game_piece_parse_host from a copy of
        its tensor."""
        L = load_library()
        tensor = None
        if isinstance(raw, (tuple, list)):
            ptr, nframes, nc, p = (int(v) for v in raw[:4])
            stride = int(raw[4]) if len(raw) > 4 else (4 + nc) * p
        else:
            tensor = raw if raw.dim() == 3 else raw[None]
            if not tensor.is_cuda or str(tensor.dtype) != "torch.float32" or tensor.dim() != 3:
                raise RuntimeError("game_piece_parse: raw must be a float32 CUDA tensor [B, 4 + C, P]")
            if tensor.stride(2) != 1 or tensor.stride(1) != tensor.shape[2]:
                tensor = tensor.contiguous()
            nframes, nc, p = tensor.shape[0], tensor.shape[1] - 4, tensor.shape[2]
            stride = tensor.stride(0) if nframes > 1 else (4 + nc) * p
            ptr = tensor.data_ptr()
        if hasattr(producer_stream, "cuda_stream"):
            producer_stream = producer_stream.cuda_stream
        limit = None if cap is None else int(cap)       # (the host route has no candidate cap of its own)
        cap = AT_GP_MAX_CANDIDATES if cap is None else int(cap)
        nf = max(int(nframes), 1)
        out = np.zeros((nf, max(cap, 1)), GP_BOX_DTYPE)
        n, status = (C.c_int * nf)(), (C.c_int * nf)()
        _check(L.at_gp_parse_device(self._h, C.c_void_p(ptr), stride, nframes, p, nc, conf, iou, int(model_size[0]),
                                    int(model_size[1]), C.c_void_p(producer_stream or 0), out.ctypes.data, cap, n,
                                    status), "at_gp_parse_device")
        res = []
        for f in range(nframes):
            if status[f] == AT_E_CAPACITY:
                if strict:
                    raise GamePieceCapacityError(f)
                host = (tensor[f].cpu().numpy() if tensor is not None
                        else self._copy_raw(ptr + 4 * stride * f, (4 + nc, p)))
                rec, _ = _gp_parse_host_frame(np.ascontiguousarray(host, np.float32), conf, iou, model_size,
                                              (self.width, self.height))
                rec = rec[:limit]
            else:
                _check(status[f], "at_gp_parse_device (frame %d)" % f)
                rec = out[f, :min(n[f], cap)].copy()
            res.append(rec if records else game_piece_boxes(rec))
        return res

    def _copy_raw(self, ptr, shape):
        """at_gp_copy_raw: a float32 array copied out of device memory on the detector's stream."""
        out = np.empty(shape, np.float32)
        _check(load_library().at_gp_copy_raw(self._h, C.c_void_p(ptr), out.ctypes.data, out.size), "at_gp_copy_raw")
        return out

    def game_piece_draw_boxes_device(self, bgr_ptr: int, boxes):
        """at_gp_draw_boxes_device: the boxes' outlines (2 px, class colour) drawn onto the
        device-resident BGR8 image at `bgr_ptr` (width x height x 3).  `boxes`: GamePieceBox
        objects or GP_BOX_DTYPE records."""
        if isinstance(boxes, np.ndarray) and boxes.dtype == GP_BOX_DTYPE:
            rec = np.ascontiguousarray(boxes)
        else:
            rec = np.array([(b.x, b.y, b.w, b.h, b.conf, b.cls) for b in boxes], GP_BOX_DTYPE)
        _check(load_library().at_gp_draw_boxes_device(self._h, rec.ctypes.data if len(rec) else None, len(rec),
                                                      C.c_void_p(bgr_ptr)), "at_gp_draw_boxes_device")

    GP_PARSE_STATS = ("candidates", "max_candidates_per_frame", "boxes", "kernels_ns")

    def game_piece_parse_stats(self):
        """at_gp_parse_stats of the last game_piece_parse."""
        buf = (C.c_uint64 * len(self.GP_PARSE_STATS))()
        n = _check(load_library().at_gp_parse_stats(self._h, buf, len(buf)), "at_gp_parse_stats")
        return dict(zip(self.GP_PARSE_STATS, [int(x) for x in buf[:n]]))

    # ---- parity taps (apriltag_gpu.h:98-183) -------------------------------
    def _copy(self, stage, frame, nbytes, dtype):
        buf = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        n = load_library().at_debug_copy(self._h, stage, frame, buf.ctypes.data, buf.nbytes)
        _check(int(n), "at_debug_copy")
        return buf[: n // np.dtype(dtype).itemsize]

    def copy_gray(self, frame=0):
        return self._copy(AT_STAGE_GRAY, frame, self.width * self.height, np.uint8).reshape(self.height, self.width)

    def copy_decimated(self, frame=0):
        return self._copy(AT_STAGE_DECIMATED, frame, self.width * self.height // 4,
                          np.uint8).reshape(self.height // 2, self.width // 2)

    def copy_thresholded(self, frame=0):
        return self._copy(AT_STAGE_THRESHOLD, frame, self.width * self.height // 4,
                          np.uint8).reshape(self.height // 2, self.width // 2)

    def copy_union_markers(self, frame=0):
        return self._copy(AT_STAGE_LABELS, frame, self.width * self.height,
                          np.uint32).reshape(self.height // 2, self.width // 2)

    def copy_union_markers_size(self, frame=0):
        return self._copy(AT_STAGE_SIZES, frame, self.width * self.height, np.uint32)

    def num_points(self, frame=0):
        return int(self._copy(AT_STAGE_NUM_POINTS, frame, 4, np.uint32)[0])

    def num_pairs(self, frame=0):
        return int(self._copy(AT_STAGE_NUM_PAIRS, frame, 4, np.uint32)[0])

    def num_pair_entries(self, frame=0):
        """Per-tile pair-histogram entries k_boundary handed to k_pairs (diagnostic)."""
        return int(self._copy(AT_STAGE_NUM_PAIR_ENTRIES, frame, 4, np.uint32)[0])

    def copy_probe(self):
        """Kernel phase clock stamps (100 MHz wall clock) written when AT_PHASE_PROBE is set."""
        return self._copy(AT_STAGE_PROBE, 0, 8 * 256, np.uint64)

    def copy_points(self, frame=0):
        """Boundary points (QuadBoundaryPoint keys), device emission order."""
        return self._copy(AT_STAGE_POINTS, frame, 8 * max(1, self.num_points(frame)), np.uint64)

    def copy_blob_points(self, frame=0):
        """IndexPoint keys of the selected blobs in (blob, theta, plane, y, x) order."""
        L = load_library()
        need = L.at_debug_copy(self._h, AT_STAGE_BLOB_POINTS, frame, C.c_void_p(1), 0)
        need = max(int(need), 8)
        return self._copy(AT_STAGE_BLOB_POINTS, frame, need, np.uint64)

    def copy_quads(self, frame=0):
        recs = (AtQuadRecord * 4096)()
        n = load_library().at_debug_copy(self._h, AT_STAGE_QUADS, frame, C.cast(recs, C.c_void_p), C.sizeof(recs))
        _check(int(n), "at_debug_copy")
        out = []
        for i in range(int(n) // C.sizeof(AtQuadRecord)):
            r = recs[i]
            out.append(dict(blob_index=r.blob_index, valid=bool(r.valid), accepted=bool(r.accepted),
                            indices=list(r.indices),
                            corners=np.array([[r.corners[k][0], r.corners[k][1]] for k in range(4)], np.float32)))
        return out


def default_cos_critical_rad():
    return math.cos(10.0 * math.pi / 180.0)
