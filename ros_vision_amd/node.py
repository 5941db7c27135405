"""Node-side adapter: the per-frame logic of the reference ROS 2 node over this
detector (reference src/apriltags_cuda/src/apriltags_cuda_detector.cu).

ROS 2 (rclpy / rclcpp, cv_bridge, image_transport) is not installed in this
image, so the adapter is transport-free: `ApriltagsDetectorNode` owns the
detector, the calibration, the extrinsics and the measurement CSV, and hands
each frame's outputs to injected publisher callables.  A ROS 2 wrapper binds
those callables to the node's publishers.  What it keeps
from the reference:

* parameters and defaults (`setup_topics`, `setup_measurement_params`,
  apriltags_cuda_detector.cu:93-133, 558-593) and the subscription QoS
  (depth 1, best effort, volatile, 50 ms deadline);
* camera calibration from ``calibrationmatrix_<serial>.json`` (`matrix`,
  `disto`, :315-371) and extrinsics from ``system_config.json``
  (`camera_mounted_positions` legacy string or ``{"location": ...}`` object,
  `extrinsics[location].rotation/offset`, :196-300);
* per frame (`imageCallback`, :382-557): detect (BGR input goes straight to the
  GPU, no CPU cvtColor), pose of every tag (GPU), camera->robot transform,
  sort by distance, the two TagDetectionArray messages (robot frame on
  `publish_pose_to_topic`, camera frame on `..._camera`), the NetworkTables
  vector ``[t, id, x, y, z] * n`` and the ``ApriltagListProto`` tag list, the
  outlined image (`draw_detection_outlines`, apriltag_utils.cu:54-79, without
  the id text), and the measurement CSV row.
"""
import json
import os
import time
from dataclasses import dataclass, field

import numpy as np

from .detector import (AT_FMT_BGR8, AT_FMT_GRAY8, AT_FMT_YUYV, TAG_SIZE, CameraMatrix, DistCoeffs, GpuDetector,
                       FieldPoseError, RigSolver, robot_in_field, tag_detections)

PARAMETER_DEFAULTS = {
    "topic_name": "camera/image_raw",
    "camera_serial": "N/A",
    "publish_images_to_topic": "apriltags/images",
    "publish_pose_to_topic": "camera/pose",
    "pin_to_core": -1,
    "priority": 80,
    "measurement_mode": False,
    "timing_csv_path": "",
}

# rclcpp::QoS(1).best_effort().durability_volatile().deadline(50 ms)
SUBSCRIPTION_QOS = {"depth": 1, "reliability": "best_effort", "durability": "volatile", "deadline_ms": 50}

CSV_HEADER = ("latency_us,det_time_us,publish_pose_us,publish_camera_pose_us,"
              "publish_image_us,networktables_us,processing_time_us")


def load_camera_calibration(calibration_dir, camera_serial):
    """calibrationmatrix_<serial>.json -> (CameraMatrix, DistCoeffs)."""
    path = os.path.join(calibration_dir, "calibrationmatrix_%s.json" % camera_serial)
    with open(path) as f:
        data = json.load(f)
    if "matrix" not in data or "disto" not in data:
        raise KeyError("calibration file %s needs 'matrix' and 'disto'" % path)
    m, d = data["matrix"], data["disto"][0]
    cam = CameraMatrix(fx=float(m[0][0]), cx=float(m[0][2]), fy=float(m[1][1]), cy=float(m[1][2]))
    dist = DistCoeffs(k1=float(d[0]), k2=float(d[1]), p1=float(d[2]), p2=float(d[3]), k3=float(d[4]))
    return cam, dist


def load_extrinsics(system_config_path, camera_serial):
    """system_config.json -> (3x3 rotation, 3 offset, location).  Identity / zero when the
    camera or its location is missing (the reference logs an error and keeps its defaults)."""
    R, t = np.eye(3), np.zeros(3)
    try:
        with open(system_config_path) as f:
            data = json.load(f)
    except (OSError, ValueError):
        return R, t, None
    pos = data.get("camera_mounted_positions", {}).get(camera_serial)
    if isinstance(pos, str):
        location = pos                      # legacy format
    elif isinstance(pos, dict) and "location" in pos:
        location = pos["location"]
    else:
        return R, t, None
    extr = data.get("extrinsics", {}).get(location)
    if not extr or "rotation" not in extr or "offset" not in extr:
        return R, t, location
    return (np.array(extr["rotation"], np.float64).reshape(3, 3), np.array(extr["offset"], np.float64).reshape(3),
            location)


def save_extrinsics(system_config_path, location, R, t):
    """Write extrinsics.<location> of system_config.json -- "rotation" 3 x 3, "offset" 3, what
    load_extrinsics reads back -- and leave the rest of the file as it was (a missing file is
    created)."""
    try:
        with open(system_config_path) as f:
            data = json.load(f)
    except OSError:
        data = {}
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    data.setdefault("extrinsics", {})[location] = {"rotation": [[float(x) for x in row] for row in R],
                                                   "offset": [float(x) for x in t]}
    with open(system_config_path, "w") as f:
        json.dump(data, f, indent=2)
        f.write("\n")


# WPILib's tag frame (x out of the face, z up, y by right-handedness) to at_pose's (x right, y
# down, z into the tag): the columns are at_pose's x, y, z axes in WPILib's frame,
# x_at = +y_wpi, y_at = -z_wpi, z_at = -x_wpi.  (The WPILib convention is written from memory,
# not checked against WPILib: DESIGN 7h.)
WPILIB_TAG_AXES = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def _quat_rotation(w, x, y, z):
    n = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _wpilib_tag(g):
    tr, q = g["pose"]["translation"], g["pose"]["rotation"]["quaternion"]
    R = _quat_rotation(float(q["W"]), float(q["X"]), float(q["Y"]), float(q["Z"])) @ WPILIB_TAG_AXES
    return g["ID"], R, [tr["x"], tr["y"], tr["z"]]


def load_field_layout(layout):
    """A field layout -- where each tag stands on the field, x_field = R x_tag + t, the tag frame
    being at_pose's -- as a list of (id, R 3x3, t 3): from such a list, or from the path of a JSON
    file, either this project's own {"tags": [{"id": 4, "R": [r00 .. r22], "t": [tx, ty, tz]}, ...]}
    or a WPILib field layout {"tags": [{"ID": 4, "pose": {"translation": {"x", "y", "z"},
    "rotation": {"quaternion": {"W", "X", "Y", "Z"}}}}, ...], "field": ...}, whose tag frame is
    turned into at_pose's (WPILIB_TAG_AXES).  The tag size is the detector's, not the file's."""
    if isinstance(layout, (str, os.PathLike)):
        with open(layout) as f:
            data = json.load(f)
        layout = [_wpilib_tag(g) if "ID" in g else (g["id"], g["R"], g["t"]) for g in data["tags"]]
    return [(int(tid), np.array(R, np.float64).reshape(3, 3), np.array(t, np.float64).reshape(3))
            for tid, R, t in layout]


def _rotation_quat(R):
    """(w, x, y, z) of a rotation matrix, w >= 0: the largest-pivot extraction, normalised."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.array(q) / np.linalg.norm(q)
    return [float(x) for x in (q if q[0] >= 0 else -q)]


def save_field_layout(path, tags, field_length=None, field_width=None):
    """Write a field layout -- (id, R, t) triples, x_field = R x_tag + t in at_pose's tag frame, e.g.
    FieldMapper's refined tags -- as the WPILib layout JSON load_field_layout reads: per tag "ID" and
    "pose" with "translation" {x, y, z} and "rotation" {"quaternion" {W, X, Y, Z}} of the tag in
    WPILib's tag frame (WPILIB_TAG_AXES undone; the same convention as load_field_layout, like it
    unchecked against WPILib), tags by ascending id, and "field" {"length", "width"} when given.
    Numbers are written with the digits that read back to the same float64, so load_field_layout
    returns t bit for bit and R as the rotation of the printed quaternion, within a few units in
    the last place of the R given.  Returns the path."""
    out = []
    for tid, R, t in sorted(load_field_layout(tags), key=lambda g: g[0]):
        w, x, y, z = _rotation_quat(R @ WPILIB_TAG_AXES.T)
        out.append({"ID": int(tid), "pose": {"translation": {"x": float(t[0]), "y": float(t[1]), "z": float(t[2])},
                                             "rotation": {"quaternion": {"W": w, "X": x, "Y": y, "Z": z}}}})
    data = {"tags": out}
    if field_length is not None or field_width is not None:
        data["field"] = {"length": float(field_length or 0.0), "width": float(field_width or 0.0)}
    with open(path, "w") as f:
        json.dump(data, f, indent=2)
        f.write("\n")
    return path


def save_camera_calibration(calibration_dir, serial, cam, dist, rms, extra=None):
    """Write calibrationmatrix_<serial>.json as the reference's calibration nodes do and
    load_camera_calibration reads it: "matrix" 3 x 3, "disto" one row of (k1, k2, p1, p2, k3),
    "rmse_reprojection_error", and "method": "apriltag_board"; `extra` (a dict) adds further keys.
    Returns the path."""
    path = os.path.join(calibration_dir, "calibrationmatrix_%s.json" % serial)
    data = {"matrix": [[float(cam.fx), 0.0, float(cam.cx)], [0.0, float(cam.fy), float(cam.cy)], [0.0, 0.0, 1.0]],
            "disto": [[float(dist.k1), float(dist.k2), float(dist.p1), float(dist.p2), float(dist.k3)]],
            "rmse_reprojection_error": float(rms), "method": "apriltag_board"}
    data.update(extra or {})
    with open(path, "w") as f:
        json.dump(data, f, indent=2)
        f.write("\n")
    return path


def grid_board(rows, cols, first_id, tag_size, pitch):
    """The layout of a printed grid of tags as CameraCalibrator's `board`: ids first_id,
    first_id + 1, ... row by row, every tag upright (R = I), the centre of the tag in row r and
    column c at (c pitch, r pitch, 0) -- x to the right and y down on the sheet, as a tag's own
    frame, the origin at the centre of the first tag.  pitch is centre to centre and must leave the
    tags apart (pitch > tag_size)."""
    if rows < 1 or cols < 1 or first_id < 0 or not tag_size > 0 or not pitch > tag_size:
        raise ValueError("grid_board: rows, cols >= 1, first_id >= 0, pitch > tag_size > 0")
    return [(int(first_id) + r * cols + c, np.eye(3), np.array([c * float(pitch), r * float(pitch), 0.0]))
            for r in range(rows) for c in range(cols)]


class CameraCalibrationCollector:
    """The reference calibration nodes' rule for taking views: a frame with a board tag counts;
    after `every` such frames in a row the current one goes to the calibrator and the count starts
    again; a frame without a board tag resets the count; `done` once max_frames views are stored."""

    def __init__(self, calibrator, every=10, max_frames=30):
        if every < 1 or max_frames < 1:
            raise ValueError("every, max_frames >= 1")
        self.calibrator, self.every, self.max_frames = calibrator, int(every), int(max_frames)
        self.run = 0
        self.board_ids = None

    @property
    def done(self):
        return len(self.calibrator) >= self.max_frames

    def offer(self, dets, board_ids=None):
        """One frame's detections.  True if the frame was stored as a view.  board_ids (a set of
        the board's ids) lets a frame count without asking the calibrator; without it every
        detection counts and the calibrator's own answer decides."""
        if self.done:
            return False
        ids = board_ids if board_ids is not None else self.board_ids
        seen = any(ids is None or d.id in ids for d in dets)
        if not seen:
            self.run = 0
            return False
        self.run += 1
        if self.run < self.every:
            return False
        self.run = 0
        return bool(self.calibrator.add(dets))


def draw_detection_outlines(bgr, dets):
    """Outline every tag on a BGR image in place: p0-p1 green, p0-p3 red, p1-p2 and p2-p3
    blue, 2 px (apriltag_utils.cu:54-79; the id text is not drawn)."""
    h, w = bgr.shape[:2]

    def line(a, b, color):
        n = int(max(abs(b[0] - a[0]), abs(b[1] - a[1]))) + 1
        xs = np.rint(np.linspace(a[0], b[0], n)).astype(int)
        ys = np.rint(np.linspace(a[1], b[1], n)).astype(int)
        for dx in (0, 1):
            for dy in (0, 1):
                x, y = xs + dx, ys + dy
                ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
                bgr[y[ok], x[ok]] = color

    for d in dets:
        p = np.asarray(d.p)
        line(p[0], p[1], (0, 255, 0))
        line(p[0], p[3], (0, 0, 255))
        line(p[1], p[2], (255, 0, 0))
        line(p[2], p[3], (255, 0, 0))
    return bgr


GAME_PIECE_PARAMETER_DEFAULTS = {   # game_piece_detection_node.cu:34-45
    "topic_name": "camera/image_raw",
    "camera_serial": "N/A",
    "engine_file": "N/A",
    "publish_to_topic": "game_piece_detector/images",
}


@dataclass
class GamePieceResult:
    """What one GamePieceDetector::imageCallback produces: the scaled detections, and the
    frame with their boxes (the reference node's image publisher, :301-307)."""
    boxes: list = field(default_factory=list)     # [GamePieceBox], class_name filled in
    image: np.ndarray = None
    image_jpeg: bytes = None
    preview_jpeg: bytes = None                    # preview_scale > 0: the scaled image with the boxes, as JPEG


def _preview_options(scale, quality, max_bytes):
    scale, quality, max_bytes = int(scale), int(quality), int(max_bytes)
    if not 0 <= scale <= 8:
        raise ValueError("preview_scale is an integer 1..8 (0: no preview)")
    if not 1 <= quality <= 100:
        raise ValueError("preview_quality is a JPEG quality, 1..100")
    if max_bytes < 0:
        raise ValueError("preview_max_bytes is a byte budget per frame (0: none)")
    return scale, quality, max_bytes


class GamePieceDetectorNode:
    """GamePieceDetector (game_piece_detection_node.cu:27-332) without the ROS transport,
    everything between the frame's upload and the boxes' download on the GPU:

    bgr8 frame -> HBM -> preprocess_image (at_gp_preprocess_device) -> `infer` -> output
    parse (at_gp_parse_device: threshold, NMS, scaling) -> boxes with class names; with an
    image topic bound (publishers[publish_to_topic], or its "/compressed" with image_jpeg)
    the boxes are drawn on the frame in HBM (at_gp_draw_boxes_device) and the image is
    copied out raw or JPEG-encoded there (at_encode_jpeg_device).

    `infer` is the user's engine: it gets the network input, a float32 CUDA torch tensor
    [1, C, H, W] on the current torch stream, and returns the output [1, 4 + classes, P]
    as a float32 CUDA tensor (produced on that stream).  input = (width, height,
    channels) of the model.

    preview_scale = 1..8 (0, the default: off): the frame scaled down by that factor with the
    boxes drawn at preview scale, JPEG-encoded on the GPU at preview_quality (lowered until the
    stream fits preview_max_bytes, if that is set; a frame nothing fits has no preview), is
    published on `<publish_to_topic>/preview/compressed` (at_preview_jpeg_device)."""

    def __init__(self, width, height, infer, input=(640, 640, 3), class_names=(), conf=0.25, iou=0.45,  # noqa: A002
                 image_jpeg=None, parameters=None, publishers=None, device=0, preview_scale=0, preview_quality=50,
                 preview_max_bytes=0):
        import torch
        self._torch = torch
        self.params = dict(GAME_PIECE_PARAMETER_DEFAULTS)
        self.params.update(parameters or {})
        self.width, self.height = int(width), int(height)
        self.infer = infer
        self.input_width, self.input_height, self.input_channels = (int(v) for v in input)
        self.class_names = list(class_names)
        self.conf, self.iou = float(conf), float(iou)
        self.image_jpeg = None if image_jpeg is None else int(image_jpeg)
        if self.image_jpeg is not None and not 1 <= self.image_jpeg <= 100:
            raise ValueError("image_jpeg is a JPEG quality, 1..100")
        self.publishers = publishers or {}
        self.image_topic = self.params["publish_to_topic"]
        self.compressed_image_topic = self.image_topic + "/compressed"
        self.preview_scale, self.preview_quality, self.preview_max_bytes = _preview_options(
            preview_scale, preview_quality, preview_max_bytes)
        self.preview_topic = self.image_topic + "/preview/compressed"
        self.detections_topic = self.image_topic.rsplit("/", 1)[0] + "/detections"
        self.device = torch.device("cuda", int(device))
        self.detector = GpuDetector(self.width, self.height, device=device, tag_size=0.0)
        self._frame = torch.empty((self.height, self.width, 3), dtype=torch.uint8, device=self.device)
        self._tensor = torch.empty((1, self.input_channels, self.input_height, self.input_width),
                                   dtype=torch.float32, device=self.device)

    def close(self):
        self.detector.close()

    def _publish(self, topic, payload):
        fn = self.publishers.get(topic)
        if fn is not None:
            fn(payload)

    def image_callback(self, image, stamp_s=0.0):
        """One bgr8 frame [H, W, 3] (cv_bridge::toCvCopy(msg, "bgr8"), :275)."""
        from .detector import game_piece_boxes, game_piece_preprocess_device
        torch = self._torch
        image = np.ascontiguousarray(image, np.uint8)
        if image.shape != (self.height, self.width, 3):
            raise ValueError("frame is %s, the node takes %s" % (image.shape, (self.height, self.width, 3)))
        stream = torch.cuda.current_stream(self.device)
        self._frame.copy_(torch.from_numpy(image), non_blocking=False)
        game_piece_preprocess_device(self._frame.data_ptr(), self.width, self.height, self._tensor.data_ptr(),
                                     self.input_width, self.input_height, self.input_channels, stream.cuda_stream)
        raw = self.infer(self._tensor)
        rec = self.detector.game_piece_parse(raw, self.conf, self.iou, (self.input_width, self.input_height),
                                             producer_stream=stream, records=True)[0]
        res = GamePieceResult(boxes=game_piece_boxes(rec, self.class_names or ()))
        if self.preview_scale:
            # (before the boxes are drawn on the frame itself; the parse waited for `stream`)
            res.preview_jpeg = _preview_or_none(lambda: self.detector.preview_jpeg_device(
                self._frame.data_ptr(), AT_FMT_BGR8, self.preview_scale, quality=self.preview_quality,
                max_bytes=self.preview_max_bytes, boxes=rec))
        want_raw, want_jpeg = self.image_topic in self.publishers, self.compressed_image_topic in self.publishers
        if (self.image_jpeg is None and want_raw) or (self.image_jpeg is not None and want_jpeg):
            # (the parse waited for `stream`: the preprocessing is done with the frame it now draws on)
            self.detector.game_piece_draw_boxes_device(self._frame.data_ptr(), rec)
            if self.image_jpeg is not None:
                res.image_jpeg = self.detector.encode_jpeg_device(self._frame.data_ptr(), quality=self.image_jpeg,
                                                                  sampling="4:2:0")
            else:
                res.image = self._frame.cpu().numpy()
        self._publish(self.detections_topic, res.boxes)
        if res.image is not None:
            self._publish(self.image_topic, res.image)
        if res.image_jpeg is not None:
            self._publish(self.compressed_image_topic, res.image_jpeg)
        if res.preview_jpeg is not None:
            self._publish(self.preview_topic, res.preview_jpeg)
        return res


def _preview_or_none(call):
    """The preview's bytes; None for a frame whose preview fits the byte budget at no quality."""
    from .detector import AT_E_CAPACITY, JpegError
    try:
        return call()[0]
    except JpegError as e:
        if e.code != AT_E_CAPACITY:
            raise
        return None


@dataclass
class FrameResult:
    """Everything one imageCallback publishes."""
    tag_detection_array: list = field(default_factory=list)          # robot frame: (id, x, y, z)
    tag_detection_camera_array: list = field(default_factory=list)   # camera frame
    networktables_pose_data: list = field(default_factory=list)      # [t, id, x, y, z] * n
    proto_tags: list = field(default_factory=list)                    # ApriltagListProto.tags
    image: np.ndarray = None
    image_jpeg: bytes = None                                          # image_jpeg set: the image as JPEG instead
    preview_jpeg: bytes = None                                        # preview_scale > 0: the scaled annotated JPEG
    field_pose: object = None          # field_layout set: the frame's FieldPose (camera in the field; n_tags 0: none)
    robot_in_field: tuple = None       # ... and (R, t) of the robot in the field, when the frame has a field pose


class ApriltagsDetectorNode:
    """ApriltagsDetector (apriltags_cuda_detector.cu) without the ROS transport."""

    def __init__(self, width, height, parameters=None, calibration_dir=None, system_config_path=None,
                 publishers=None, device=0, mjpg_color=False, image_jpeg=None, mjpg_device_entropy=False,
                 preview_scale=0, preview_quality=50, preview_max_bytes=0, field_layout=None, field_max_hamming=0,
                 undistort=False):
        self.params = dict(PARAMETER_DEFAULTS)
        self.params.update(parameters or {})
        serial = self.params["camera_serial"]
        if calibration_dir is not None:
            cam, dist = load_camera_calibration(calibration_dir, serial)
        else:
            from .detector import TEST_CAMERA, TEST_DIST
            cam, dist = TEST_CAMERA, TEST_DIST
        self.camera, self.distortion = cam, dist
        self.extrinsic_rotation, self.extrinsic_offset, self.location = (
            load_extrinsics(system_config_path, serial) if system_config_path else (np.eye(3), np.zeros(3), None))
        self.detector = GpuDetector(width, height, cam, dist, device=device, tag_size=TAG_SIZE)
        # "jpeg" frames: also decode colour on the GPU and publish the annotated image
        self.mjpg_color = bool(mjpg_color)
        if self.mjpg_color:
            self.detector.set_mjpg_color(True)
        # "jpeg" frames: the GPU decodes the entropy-coded data too (the host parses markers only)
        self.mjpg_device_entropy = bool(mjpg_device_entropy)
        if self.mjpg_device_entropy:
            self.detector.set_mjpg_device_entropy(True)
        self.publishers = publishers or {}
        self.pose_topic = self.params["publish_pose_to_topic"]
        self.camera_pose_topic = self.pose_topic + "_camera"
        self.image_topic = self.params["publish_images_to_topic"]
        # image_jpeg = <quality 1..100>: the annotated image is drawn and JPEG-encoded on the GPU
        # (at_annotate_jpeg, 4:2:0 as cv::imencode writes) and published as bytes on the
        # compressed topic, the one the bag recording and the viewer read, instead of raw
        self.image_jpeg = None if image_jpeg is None else int(image_jpeg)
        if self.image_jpeg is not None and not 1 <= self.image_jpeg <= 100:
            raise ValueError("image_jpeg is a JPEG quality, 1..100")
        self.compressed_image_topic = self.image_topic + "/compressed"
        # preview_scale = 1..8 (0: off): the frame of ANY encoding scaled down by that factor on the
        # GPU, annotated at preview scale and JPEG-encoded at preview_quality -- lowered until the
        # stream fits preview_max_bytes, if set -- on <publish_images_to_topic>/preview/compressed
        self.preview_scale, self.preview_quality, self.preview_max_bytes = _preview_options(
            preview_scale, preview_quality, preview_max_bytes)
        self.preview_topic = self.image_topic + "/preview/compressed"
        # field_layout = [(id, R, t), ...] or the path of a layout JSON (load_field_layout): the GPU
        # also solves every frame's camera pose from all its layout tags (k_field), and the robot's
        # pose in the field -- (R, t), x_field = R x_robot + t -- goes out on <publish_pose_to_topic>/field
        self.field_layout = load_field_layout(field_layout) if field_layout is not None else None
        self.field_pose_topic = self.pose_topic + "/field"
        if self.field_layout:
            self.detector.set_field_layout(self.field_layout, field_max_hamming)
        # undistort: the tag, field and rig poses from ideal corners -- the lens distortion of the
        # calibration file undone on the GPU (at_set_undistort); the detections and drawings stay raw
        self.undistort = bool(undistort)
        if self.undistort:
            self.detector.set_undistort(True)
        self.csv = None
        if self.params["measurement_mode"]:
            path = self.params["timing_csv_path"] or time.strftime("apriltags_timing_%Y%m%d_%H%M%S.csv")
            self.csv = open(path, "w")
            self.csv.write(CSV_HEADER + "\n")
            self.csv.flush()

    def close(self):
        if self.csv:
            self.csv.close()
            self.csv = None
        self.detector.close()

    def _publish(self, topic, payload):
        fn = self.publishers.get(topic)
        if fn is not None:
            fn(payload)

    def image_callback(self, image, stamp_s, encoding="bgr8", receive_time_s=None):
        """One frame: `image` is bgr8 [H, W, 3] (what cv_bridge hands the reference),
        yuyv [H, 2W], mono8 [H, W], or -- encoding "jpeg" -- the bytes of one MJPG camera
        frame (a sensor_msgs/CompressedImage's data): its luma is decoded on the way to
        the GPU, poses and tables come out as for the other encodings.  An annotated
        image is published for it only with mjpg_color=True: the frame's colour is then
        decoded on the GPU too and outlined there (at_annotate_staged); otherwise there is
        no colour image to draw on.  With image_jpeg set, whichever image there is goes out
        as JPEG bytes on `<publish_images_to_topic>/compressed` and the raw topic is silent.
        With preview_scale > 0 every encoding -- yuyv, mono8 and jpeg without colour included --
        also gets the scaled annotated JPEG on `<publish_images_to_topic>/preview/compressed`."""
        start = time.perf_counter()
        latency_s = (receive_time_s if receive_time_s is not None else time.time()) - stamp_s
        det0 = time.perf_counter()
        if encoding == "jpeg":
            dets = self.detector.detect_mjpg(bytes(image))
        else:
            fmt = {"bgr8": AT_FMT_BGR8, "mono8": AT_FMT_GRAY8}.get(encoding, AT_FMT_YUYV)
            dets = self.detector.detect(np.ascontiguousarray(image), fmt)
        det1 = time.perf_counter()
        poses = self.detector.poses()
        res = FrameResult()
        for tag in tag_detections(poses, self.extrinsic_rotation, self.extrinsic_offset):
            rx, ry, rz = (float(v) for v in tag.robot)
            res.networktables_pose_data += [stamp_s, tag.id * 1.0, rx, ry, rz]
            res.proto_tags.append({"collect_time": stamp_s, "tag_id": tag.id, "x": rx, "y": ry, "z": rz})
            res.tag_detection_camera_array.append((tag.id, *(float(v) for v in tag.camera)))
            res.tag_detection_array.append((tag.id, rx, ry, rz))
        if self.field_layout:
            res.field_pose = self.detector.field_poses()[0]
            if res.field_pose.n_tags:
                res.robot_in_field = robot_in_field(res.field_pose, self.extrinsic_rotation, self.extrinsic_offset)
        if self.preview_scale:
            # (first: at_annotate_staged / at_annotate_jpeg below draw on the staged frame itself)
            res.preview_jpeg = _preview_or_none(lambda: self.detector.preview_jpeg(
                0, self.preview_scale, quality=self.preview_quality, max_bytes=self.preview_max_bytes))
        has_image = encoding == "bgr8" or (encoding == "jpeg" and self.mjpg_color)
        if has_image and self.image_jpeg is not None:
            res.image_jpeg = self.detector.annotate_jpeg(0, quality=self.image_jpeg, sampling="4:2:0")
        elif encoding == "bgr8":
            res.image = draw_detection_outlines(np.array(image, copy=True), dets)
        elif has_image:
            res.image = self.detector.annotate_staged(0)
        nt0 = time.perf_counter()
        self._publish("networktables", res.networktables_pose_data)
        self._publish("networktables_proto", res.proto_tags)
        nt1 = time.perf_counter()
        self._publish(self.pose_topic, res.tag_detection_array)
        pp1 = time.perf_counter()
        self._publish(self.camera_pose_topic, res.tag_detection_camera_array)
        if res.robot_in_field is not None:
            self._publish(self.field_pose_topic, res.robot_in_field)
        pc1 = time.perf_counter()
        if res.image is not None:
            self._publish(self.image_topic, res.image)
        if res.image_jpeg is not None:
            self._publish(self.compressed_image_topic, res.image_jpeg)
        if res.preview_jpeg is not None:
            self._publish(self.preview_topic, res.preview_jpeg)
        pi1 = time.perf_counter()
        if self.csv:
            us = lambda a, b: int(round((b - a) * 1e6))  # noqa: E731
            self.csv.write("%d,%d,%d,%d,%d,%d,%d\n" % (int(latency_s * 1e6), us(det0, det1), us(nt1, pp1),
                                                       us(pp1, pc1), us(pc1, pi1), us(nt0, nt1), us(start, pi1)))
            self.csv.flush()
        return res



class RigPoseFuser:
    """One robot pose per instant from every camera of the robot: a RigSolver over the detectors
    and loaded extrinsics of several ApriltagsDetectorNodes (all of this process, one device).
    After the nodes' image_callbacks for one instant, publish() solves and sends (R, t, cov) --
    x_field = R x_robot + t, cov 6 x 6 in (w, t) order (RigPose) -- on
    <publish_pose_to_topic>/rig of the first node; an instant without a layout tag sends nothing.
    With a `calibrator` (RigCalibrator over the same cameras, in the nodes' order) every fused
    instant is also added to it, from the nodes' collected detections and poses.
    With a `tracker` (RigTracker over the same cameras, in the nodes' order) every instant is pushed
    to it -- one without a tag too, which its odometry holds -- and the smoothed latest (R, t, cov)
    (RigTrack) goes out on <publish_pose_to_topic>/rig/tracked.
    A node created with undistort=True hands its ideal detections on (k_rig reads them on the
    device; the calibrator and the tracker get ideal_detections(0)), the others their raw ones.
    With `robust` (a RigRobust) the published record is RigSolver.solve_robust's, its RigRobustInfo
    is kept in self.robust_info, and the calibrator and the tracker get the frames without the
    detections (and their poses) of the tags that solve dropped."""

    def __init__(self, camera_nodes, field_layout, max_hamming=0, publishers=None, calibrator=None, tracker=None,
                 robust=None):
        self.nodes = list(camera_nodes)
        self.field_layout = load_field_layout(field_layout)
        self.solver = RigSolver([n.detector for n in self.nodes],
                                [(n.extrinsic_rotation, n.extrinsic_offset) for n in self.nodes],
                                self.field_layout, max_hamming)
        self.publishers = publishers if publishers is not None else self.nodes[0].publishers
        self.rig_pose_topic = self.nodes[0].pose_topic + "/rig"
        self.calibrator = calibrator
        self.tracker = tracker
        self.tracked_pose_topic = self.rig_pose_topic + "/tracked"
        self.tracked = None
        self.robust = robust
        self.robust_info = None

    def close(self):
        self.solver.close()

    def frames(self, info=None):
        """(detections, poses) of the instant per node: ideal detections where the node undistorts.
        With `info`, the RigRobustInfo of a robust solve of this same instant (publish() passes its
        own), without the tags that solve dropped: per camera every detection of a dropped id goes,
        a second detection of that id which the selection passed over too -- it is the tag that is
        wrong, and the next selection would pick that one up."""
        out = [(n.detector.ideal_detections(0) if getattr(n.detector, "undistort", False) else n.detector.detections(0),
                n.detector.poses(0)) for n in self.nodes]
        if info is None:
            return out
        kept = []
        for (dets, poses), gone in zip(out, info.dropped):
            keep = [i for i, d in enumerate(dets) if d.id not in gone]
            kept.append(([dets[i] for i in keep], [poses[i] for i in keep]))
        return kept

    def publish(self, odometry=None, stamp_s=0.0):
        """The RigPose of the instant the nodes last saw (published when it has a tag).  With a
        tracker: `odometry` is RigTracker.push's (None: a new chain), `stamp_s` the instant's time;
        the tracked pose is kept in self.tracked (None while the window has no tag)."""
        if self.robust is not None:
            pose, self.robust_info = self.solver.solve_robust(self.robust)[0]
        else:
            pose = self.solver.solve()[0]
        if pose.n_tags:
            fn = self.publishers.get(self.rig_pose_topic)
            if fn is not None:
                fn((pose.R, pose.t, pose.cov))
        # (the frames of the instant just solved, filtered by that solve's own info)
        handed = self.frames(self.robust_info) if self.calibrator is not None or self.tracker is not None else None
        if self.calibrator is not None:
            self.calibrator.add(handed)
        if self.tracker is not None:
            self.tracker.push(handed, odometry, stamp_s)
            try:
                self.tracked = self.tracker.solve()
            except FieldPoseError:  # (no tag anywhere in the window yet)
                self.tracked = None
            fn = self.publishers.get(self.tracked_pose_topic)
            if self.tracked is not None and fn is not None:
                fn((self.tracked.R, self.tracked.t, self.tracked.cov))
        return pose
