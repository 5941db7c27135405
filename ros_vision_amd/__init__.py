"""MI355X-native AprilTag detection stage (drop-in for ros_vision's apriltags_cuda detector).

Product code: HIP kernels + C ABI in ``csrc/`` (built into ``libat_hip.so``),
the Python mirror of the reference GpuDetector interface in ``detector.py``
and the synthetic tag-board generator in ``synth.py``.
"""
from .detector import (AT_FMT_BGR8, AT_FMT_GRAY8, AT_FMT_YUYV, TAG_SIZE, TEST_CAMERA, TEST_DIST,  # noqa: F401
                       CameraMatrix, Detection, DistCoeffs, GpuDetector, JpegError, Pose, TagDetection, family_entries,
                       MjpgError, game_piece_preprocess_device, jpeg_encode_host, jpeg_max_bytes, load_library,
                       mjpg_decode_bgr, mjpg_decode_gray, mjpg_dense_host, mjpg_entropy_host, mjpg_stream_mode,
                       tag_detections,
                       AT_GP_MAX_CANDIDATES, GP_BOX_DTYPE, GamePieceBox, GamePieceCapacityError, game_piece_boxes,
                       game_piece_parse_host, preview_host, preview_jpeg_host, preview_size,
                       FieldPose, FieldPoseError, field_pose_host, robot_in_field,
                       AT_RIG_MAX_CAMS, RigPose, RigSolver, rig_pose_host, RigRobust, RigRobustInfo, rig_pose_robust_host,
                       AT_RIGCAL_MAX_INSTANTS, RigCalibration, RigCalibrator, RigCalInstant,
                       AT_RIGTRACK_MAX_WINDOW, RigTrack, RigTracker, RigTrackInstant,
                       AT_CAMCAL_ALL, AT_CAMCAL_CX, AT_CAMCAL_CY, AT_CAMCAL_FX, AT_CAMCAL_FY, AT_CAMCAL_K1, AT_CAMCAL_K2,
                       AT_CAMCAL_K3, AT_CAMCAL_MAX_VIEWS, AT_CAMCAL_P1, AT_CAMCAL_P2, AT_CAMCAL_PINHOLE, CAMCAL_PARAMS,
                       CameraCalibration, CameraCalibrator, CameraCalView,
                       AT_FIELDMAP_MAX_TAGS, AT_FIELDMAP_MAX_VIEWS, FieldMap, FieldMapper, FieldMapTag, FieldMapView,
                       ideal_detections_host, undistort_points_host)

__all__ = ["GpuDetector", "CameraMatrix", "DistCoeffs", "Detection", "Pose", "TagDetection", "load_library",
           "family_entries", "tag_detections", "game_piece_preprocess_device", "TAG_SIZE", "TEST_CAMERA", "TEST_DIST",
           "AT_FMT_YUYV", "AT_FMT_BGR8", "AT_FMT_GRAY8", "MjpgError", "mjpg_decode_gray", "mjpg_stream_mode",
           "mjpg_decode_bgr", "mjpg_dense_host", "mjpg_entropy_host", "JpegError", "jpeg_encode_host", "jpeg_max_bytes",
           "GamePieceBox", "GamePieceCapacityError", "game_piece_parse_host", "game_piece_boxes", "GP_BOX_DTYPE",
           "AT_GP_MAX_CANDIDATES", "preview_size", "preview_host", "preview_jpeg_host",
           "FieldPose", "FieldPoseError", "field_pose_host", "robot_in_field",
           "AT_RIG_MAX_CAMS", "RigPose", "RigSolver", "rig_pose_host", "RigRobust", "RigRobustInfo",
           "rig_pose_robust_host",
           "AT_RIGCAL_MAX_INSTANTS", "RigCalibration", "RigCalibrator", "RigCalInstant",
           "AT_RIGTRACK_MAX_WINDOW", "RigTrack", "RigTracker", "RigTrackInstant",
           "AT_CAMCAL_MAX_VIEWS", "AT_CAMCAL_FX", "AT_CAMCAL_FY", "AT_CAMCAL_CX", "AT_CAMCAL_CY", "AT_CAMCAL_K1",
           "AT_CAMCAL_K2", "AT_CAMCAL_P1", "AT_CAMCAL_P2", "AT_CAMCAL_K3", "AT_CAMCAL_PINHOLE", "AT_CAMCAL_ALL",
           "CAMCAL_PARAMS", "CameraCalibration", "CameraCalibrator", "CameraCalView",
           "AT_FIELDMAP_MAX_TAGS", "AT_FIELDMAP_MAX_VIEWS", "FieldMap", "FieldMapper", "FieldMapTag", "FieldMapView",
           "ideal_detections_host", "undistort_points_host"]
