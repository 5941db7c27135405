/*
 * at_api.h -- C ABI of the MI355X-native AprilTag detection stage.
 *
 * Drop-in boundary for the reference's per-frame detector
 * frc971::apriltag::GpuDetector (Team766/ros_vision,
 * src/apriltags_cuda/include/apriltags_cuda/apriltag_gpu.h:77-359), whose
 * caller is ApriltagsDetector::imageCallback
 * (src/apriltags_cuda/src/apriltags_cuda_detector.cu:382-557).  Plain C types
 * only; every entry point returns 0 or a negative AT_E* code (the reference
 * aborts through glog CHECK instead, cuda_frc971.h:14-17).
 *
 * Threading: one at_detector per camera stream (the reference owns one
 * GpuDetector + one CUDA stream per node, apriltag_gpu.h:240); calls on one
 * instance must not overlap.
 */
#ifndef AT_API_H_
#define AT_API_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AT_ABI_VERSION 8

enum {
  AT_OK = 0,
  AT_E_INVALID = -1,    /* bad argument / unsupported geometry */
  AT_E_HIP = -2,        /* HIP runtime error (no device, launch failure) */
  AT_E_CAPACITY = -3,   /* frame exceeded a fixed capacity (see at_frame_status) */
  AT_E_FAMILY = -4,     /* unknown tag family */
  AT_E_NOMEM = -5,
  AT_E_UNSUPPORTED = -6 /* a JPEG stream the MJPG path does not decode (see at_enqueue_mjpg) */
};

typedef struct at_detector at_detector; /* opaque: device buffers + hipStream_t */

typedef enum { AT_FMT_YUYV = 0, AT_FMT_BGR8 = 1, AT_FMT_GRAY8 = 2 } at_pixfmt;

/* CameraMatrix + DistCoeffs (apriltag_gpu.h:61-74), read from
 * calibrationmatrix_<serial>.json by apriltags_cuda_detector.cu:315-371. */
typedef struct {
  double fx, fy, cx, cy;
  double k1, k2, p1, p2, k3;
} at_camera;

/* apriltag_detector_t fields the reference consults
 * (apriltags_cuda_detector.cu:139-147; apriltag_gpu.cu:166-181, 737, 884, 1084-1086). */
typedef struct {
  int width, height;          /* frame size; width%8==0, height%8==0, width*height < 2^22 */
  const char *family;         /* "tag36h11" (apriltags_cuda_detector.hpp:213), "tag25h9", "tag16h5";
                                 the apriltag 3 layouts give AT_E_FAMILY (apriltag_utils.cu:10-32) */
  float quad_decimate;        /* must be 2.0 (apriltag_gpu.cu:166) */
  int refine_edges;           /* 1 */
  double decode_sharpening;   /* 0.25 */
  int min_white_black_diff;   /* 5 */
  int min_cluster_pixels;     /* 5 */
  int max_nmaxima;            /* must be 10 (line_fit_filter.cu:1205) */
  float max_line_fit_mse;     /* 10.0 */
  double cos_critical_rad;    /* cos(10 deg) */
  int device;                 /* HIP device ordinal */
  int max_batch;              /* frames per at_detect_batch / at_detect_device call (1..256) */
  double tag_size;            /* metres; > 0 also estimates every tag's pose on the GPU
                                 (info_.tagsize = TAGSIZE 0.1651, apriltags_cuda_detector.cu:185,
                                 apriltags_cuda_detector.hpp:39); 0 = detection only */
} at_config;

/* apriltag_detection_t fields published downstream (apriltag.h; consumed at
 * apriltags_cuda_detector.cu:425-496). */
typedef struct {
  int32_t id;
  int32_t hamming;
  float decision_margin;
  double H[9];      /* row-major 3x3 homography, tag [-1,1]^2 -> pixels */
  double c[2];      /* centre */
  double p[4][2];   /* corners */
} at_detection;

/* Fills the reference defaults for a width x height camera. */
int at_config_default(at_config *cfg, int width, int height);

/* GpuDetector::GpuDetector (apriltag_gpu.cu:111-188): allocates every buffer
 * at worst-case size for max_batch frames; nothing is allocated per frame. */
int at_create(const at_config *cfg, const at_camera *cam, at_detector **out);

/* GpuDetector::Detect + Detections (apriltag_gpu.cu:725-1166,
 * apriltag_detect.cu:618-663): one host frame in, detections sorted by id out.
 * *n receives the total found; at most cap are written. Synchronous. */
int at_detect(at_detector *d, const uint8_t *frame, at_pixfmt fmt, at_detection *out, int cap, int *n);

/* Batched host frames (one launch sequence for all frames; multi-camera). */
int at_detect_batch(at_detector *d, const uint8_t *const *frames, int nframes, at_pixfmt fmt,
                    at_detection *out, int cap_per_frame, int *n_per_frame);

/* Frames already resident in device memory: d_frames is a device pointer to
 * nframes frames laid out back to back (frame_stride bytes apart).  The kernels
 * read the frames until the last stage (the decode samples luma from YUYV / GRAY8
 * frames in place), so the buffer must stay unmodified until the call returns --
 * for at_enqueue_device, until at_collect returns. */
int at_detect_device(at_detector *d, const void *d_frames, size_t frame_stride, int nframes, at_pixfmt fmt,
                     at_detection *out, int cap_per_frame, int *n_per_frame);

/* Split-phase form of at_detect_device for pipelining: enqueue the batch on
 * the detector's stream and return immediately; at_collect waits for it and
 * runs the host tail (reconcile + sort by id).  d_frames must stay unmodified
 * until at_collect returns (see at_detect_device): a producer that reuses the
 * buffer must order its writes after at_collect, not after earlier work. */
int at_enqueue_device(at_detector *d, const void *d_frames, size_t frame_stride, int nframes, at_pixfmt fmt);
int at_collect(at_detector *d, at_detection *out, int cap_per_frame, int *n_per_frame);
/* Split-phase form of at_detect_batch (camera-fed pipelines): the host-to-device
 * copies of the frames (one per run of back-to-back frames; page-locked sources,
 * e.g. hipHostMalloc'd or registered, copy asynchronously) and the batch are
 * enqueued on the detector's stream, so with several detectors in turn the copies
 * of one batch overlap the kernels of another.  The frames must stay untouched
 * until at_collect. */
int at_enqueue_host(at_detector *d, const uint8_t *const *frames, int nframes, at_pixfmt fmt);

/* MJPG camera frames (what every camera of the deployed configuration delivers).
 * Each frame is one baseline sequential 8-bit Huffman JPEG (SOF0) of the detector's
 * size: 3 components 4:4:4, 4:2:2 or 4:2:0 in one interleaved scan, or 1 component;
 * DRI / RSTn restarts; APPn (the AVI1 APP0 of UVC cameras) and COM are skipped; a
 * stream without DHT segments is decoded with the standard Annex K tables.  Only luma
 * is decoded: the host does the Huffman decode and sends the quantised luma
 * coefficients (at most 2 B per pixel, typically well under 1), the GPU dequantises,
 * runs the inverse DCT and writes the GRAY8 plane the detection then reads.  The plane
 * equals libjpeg's integer "slow" IDCT luma bit for bit.
 *
 * at_enqueue_mjpg first parses and entropy-decodes every frame on the host.  If one
 * fails, nothing is enqueued, the detector (a pending batch included) is as before,
 * *bad_frame (may be NULL) is its index and the code is returned: AT_E_UNSUPPORTED for
 * progressive, arithmetic-coded, 12-bit, 4-component or otherwise sampled streams,
 * AT_E_INVALID for malformed or truncated ones and for a size other than the
 * detector's.  Otherwise it continues like at_enqueue_host with GRAY8 frames;
 * at_collect, at_poses, at_detections, at_frame_status and at_debug_copy follow as
 * usual (AT_STAGE_GRAY with the taps on is the decoded plane).  at_annotate_staged
 * after an MJPG batch is AT_E_INVALID unless colour was on (at_mjpg_set_color): there
 * is no chroma on the device then.
 * The host decode waits for nothing, so called while the batch before is still running
 * it overlaps that batch (two staging sets); like every enqueue it then waits for a
 * batch not yet collected before it reuses the result buffers.
 * The jpgs need to stay valid only until the call returns. */
int at_enqueue_mjpg(at_detector *d, const uint8_t *const *jpgs, const size_t *lens, int nframes, int *bad_frame);
int at_detect_mjpg(at_detector *d, const uint8_t *jpg, size_t len, at_detection *out, int cap, int *n);
int at_detect_mjpg_batch(at_detector *d, const uint8_t *const *jpgs, const size_t *lens, int nframes,
                         at_detection *out, int cap_per_frame, int *n_per_frame, int *bad_frame);
/* Host threads that decode the frames of one MJPG batch (default 1; clamped to 1..16). */
int at_mjpg_set_threads(at_detector *d, int n);
/* The last enqueued MJPG batch: [0] compressed bytes in, [1] bytes sent to the device,
 * [2] frames sent in the dense encoding, [3] host parse + decode time, microseconds,
 * [4] k_mjpg_idct's time in nanoseconds (HIP events; measured while at_set_profiling
 * is on and known once the batch is collected, 0 otherwise).
 * Returns the number of entries written. */
int at_mjpg_stats(at_detector *d, uint64_t *out, int cap);
/* Colour (off by default; takes effect from the next at_enqueue_mjpg): the host keeps the
 * Cb and Cr coefficients too and sends them behind the luma ones (each component with
 * its own quantisation table), the GPU runs the same IDCT on the two chroma planes,
 * upsamples them (libjpeg's "fancy" triangle filter for 4:2:2 and 4:2:0) and converts
 * to BGR8.  The image equals libjpeg-turbo's default decode bit for bit (a
 * single-component frame gives B = G = R = Y).  The detection reads the same luma plane
 * as with colour off.  After a batch enqueued with colour on:
 *   at_mjpg_bgr gives frame `frame`'s BGR8 image (width x height x 3, row-major) in device
 *   memory, valid until the next batch (the no-copy hand-off, like at_gp_tensor);
 *   at_mjpg_copy_bgr copies it to the host (cap >= width * height * 3);
 *   at_annotate_staged draws on that image and copies it out (it is consumed);
 *   with at_gp_enable, at_gp_tensor / at_gp_copy serve the batch's game-piece tensors,
 *   computed from those images.
 * Both return AT_E_INVALID unless the last batch was such a batch (whatever the setting
 * is now) and `frame` is one of its frames.  at_mjpg_stats [5]: the time of the two
 * colour kernels (chroma IDCT, upsampling + conversion) in nanoseconds, measured like [4]. */
int at_mjpg_set_color(at_detector *d, int enable);
int at_mjpg_bgr(at_detector *d, int frame, const uint8_t **dev_ptr);
int at_mjpg_copy_bgr(at_detector *d, int frame, uint8_t *dst, size_t cap);
/* Host only, no device needed: the full luma decode of one such JPEG (any size up to
 * 2^26 pixels) with the same integer IDCT the kernel runs -- the CPU reference of the
 * MJPG path.  *w / *h (may be NULL) receive the picture size; gray == NULL parses the
 * frame header only.  at_mjpg_stream_mode_host tells how the frame would travel to a
 * want_w x want_h detector (0, 0: any size): 0 sparse, 1 dense, < 0 the error
 * at_enqueue_mjpg would return; *stream_bytes (may be NULL) its size on the link (with
 * colour off).  at_mjpg_decode_bgr_host is the full colour decode to BGR8 (cap >= 3 * w * h)
 * through the arithmetic the colour kernels share -- their CPU reference. */
int at_mjpg_decode_gray_host(const uint8_t *jpg, size_t len, uint8_t *gray, size_t cap, int *w, int *h);
int at_mjpg_decode_bgr_host(const uint8_t *jpg, size_t len, uint8_t *bgr, size_t cap, int *w, int *h);
int at_mjpg_stream_mode_host(const uint8_t *jpg, size_t len, int want_w, int want_h, size_t *stream_bytes);

/* Entropy decode on the GPU (off by default; takes effect from the next at_enqueue_mjpg).
 * With it on, at_enqueue_mjpg only parses each frame's markers on the host (SOI .. SOS, the
 * quantisation and Huffman tables, Annex K defaults included, the size and sampling checks:
 * the structural refusals, *bad_frame and "nothing enqueued" are exactly those above) and
 * sends the frame as it is: the stream headers, a table block (the decode tables the scan
 * names and its geometry, at most 9.4 KB) and the raw scan bytes, stuffing and RSTn markers
 * still in.  k_mjpg_entropy then decodes the scan in parallel -- each thread a piece of S
 * bytes, the threads exchanging entry states until nothing changes, which is within
 * `pieces` rounds and gives the serial decode exactly -- and leaves the dense coefficient
 * layout k_mjpg_idct and the colour kernels read; nothing returns to the host in between.
 * Colour (at_mjpg_set_color) works as with the switch off.
 *   A frame whose scan data exceeds width * height bytes takes the host route inside the
 * same batch (decoded and packed by the host as with the switch off): no frame fails for
 * size.
 *   Errors in the entropy-coded data (a code no table has, a run past coefficient 63, bits
 * needed from beyond the data, a wrong or missing RSTn, too few blocks) are only seen on
 * the device.  at_enqueue_mjpg succeeds; all coefficients of such a frame are left zero, so
 * its plane is a flat 128 and it has no detections; at_frame_status gives AT_E_INVALID for
 * it and at_collect returns AT_E_INVALID (in front of AT_E_CAPACITY) while the other
 * frames' results stay valid.  The streams accepted are exactly those the host decoder
 * accepts.
 *   at_mjpg_stats gains [6] the time of k_mjpg_entropy in nanoseconds (measured like [4]),
 * [7] frames that took the host route, [8] the most synchronisation rounds a frame of the
 * batch needed (known once the batch is collected); with the switch on [1] counts the bytes
 * that crossed the link.  Callers passing cap 6 see no change.
 *   at_mjpg_set_subseq sets S (a power of two from 16 to 256 bytes, default 128; a tuning
 * aid, AT_E_INVALID otherwise). */
int at_mjpg_set_device_entropy(at_detector *d, int enable);
int at_mjpg_set_subseq(at_detector *d, int bytes);
/* Host only: the same parallel algorithm run sequentially over the pieces -- the CPU
 * reference of k_mjpg_entropy.  Writes the frame's dense coefficient streams (headers and
 * payloads; with keep_chroma the Cb / Cr sub-streams) to out; *rounds (may be NULL) is the
 * number of synchronisation rounds.  at_mjpg_dense_host writes what the serial host decoder
 * gives in the same layout (out == NULL: only *out_bytes, the size of either). */
int at_mjpg_entropy_host(const uint8_t *jpg, size_t len, int want_w, int want_h, int subseq_bytes, int keep_chroma,
                         uint8_t *out, size_t cap, int *rounds);
int at_mjpg_dense_host(const uint8_t *jpg, size_t len, int want_w, int want_h, int keep_chroma, uint8_t *out,
                       size_t cap, size_t *out_bytes);

/* Stream ordering without a host wait: the detector's next enqueued batch starts
 * only after everything queued so far on `stream` (a hipStream_t of the same
 * device, e.g. the stream a frame scatter or copy was issued on; NULL = the null
 * stream) has completed.  Replaces a host synchronize between a producer of
 * device-resident frames and at_enqueue_device. */
int at_stream_wait(at_detector *d, void *stream);

/* Per-frame status of the last batch: 0 or AT_E_CAPACITY (a frame whose blob
 * pair count exceeded the reference's 12-bit blob index, points.h:183-193); after an MJPG
 * batch with the device entropy decode on, AT_E_INVALID for a frame whose entropy-coded
 * data was bad (at_mjpg_set_device_entropy). */
int at_frame_status(at_detector *d, int frame);

/* Per-stage parity taps (the reference's Copy*To debug accessors,
 * apriltag_gpu.h:98-183).  Copies the named stage of frame `frame` of the
 * last batch into dst (host memory). Returns bytes copied or < 0. */
enum {
  AT_STAGE_GRAY = 0,        /* u8  [H][W] */
  AT_STAGE_DECIMATED = 1,   /* u8  [H/2][W/2] */
  AT_STAGE_THRESHOLD = 2,   /* u8  [H/2][W/2] in {0,127,255} */
  AT_STAGE_LABELS = 3,      /* u32 [H/2][W/2] */
  AT_STAGE_SIZES = 4,       /* u32 [H/2 * W/2] */
  AT_STAGE_NUM_POINTS = 5,  /* u32 count of boundary points N_c */
  AT_STAGE_NUM_PAIRS = 6,   /* u32 count of blob pairs N_q */
  AT_STAGE_QUADS = 7,       /* at_quad_record[] of fitted quads (see below) */
  AT_STAGE_POINTS = 8,      /* u64 QuadBoundaryPoint keys, in emission order (unordered) */
  AT_STAGE_BLOB_POINTS = 9, /* u64 IndexPoint keys of selected blobs, sorted (blob, theta) */
  AT_STAGE_NUM_PAIR_ENTRIES = 10, /* u32 per-tile pair-histogram entries (diagnostic) */
  AT_STAGE_PROBE = 11       /* u64[256] kernel phase clock stamps when AT_PHASE_PROBE is set (diagnostic) */
};
long long at_debug_copy(at_detector *d, int stage, int frame, void *dst, size_t bytes);
/* AT_STAGE_GRAY: the full-resolution gray plane is written for BGR8 batches (k_decode
 * samples it) and, for YUYV / GRAY8 batches, only while the debug taps are on (k_decode
 * then reads the frame's own luma); AT_E_INVALID otherwise.
 * AT_STAGE_BLOB_POINTS needs the blob kernels to write the sorted IndexPoint keys
 * back (8 B per point of every selected blob): off by default (production), on
 * with at_set_debug_taps(d, 1) for parity checks; AT_E_INVALID while off.
 * AT_STAGE_SIZES of a throughput-mode batch (max_batch >= 8) likewise needs the taps
 * (that mode carries the size test in the root words, not in the size plane), and so
 * does AT_STAGE_QUADS (the fitted-quad records are debug output only). */
int at_set_debug_taps(at_detector *d, int enable);

/* Fitted quad record (FitQuad + QuadCorners, line_fit_filter.h:130-135 and
 * apriltag_gpu.h:55-59). */
typedef struct {
  uint32_t blob_index;
  uint32_t valid;          /* FitQuads valid flag */
  uint32_t accepted;       /* passed UpdateFitQuads checks */
  uint16_t indices[4];
  float corners[4][2];     /* after AdjustPixelCenters (full resolution) */
} at_quad_record;

/* Per-stage GPU timing with HIP events between the kernels of the launch
 * sequence (the reference times every stage with CudaEvents and logs them at
 * VLOG(1), apriltag_gpu.cu:1118-1163).  at_stage_times writes the mean
 * milliseconds per batch of each stage to ms[0..n-1] and the number of timed
 * batches to ms[n]; returns n (the stage count) or < 0. */
int at_set_profiling(at_detector *d, int enable);
int at_stage_times(at_detector *d, double *ms, int cap);
const char *at_stage_name(int stage);

/* Live per-launch time of ONE kernel (stage index as at_stage_name) inside
 * the normal launch sequence (concurrent streams; direct launches instead of
 * the graph replay while a timer is set): HIP events bracket that kernel on
 * its own stream.  stage -1 switches it off.
 * at_kernel_time: mean ms per launch and number of launches since set. */
int at_set_kernel_timer(at_detector *d, int stage);
int at_kernel_time(at_detector *d, double *avg_ms, long long *launches);
/* The same launches timed on the device: first workgroup's start to last
 * workgroup's end on the GPU wall clock (the kernel's execution span, as a
 * rocprofv3 kernel trace measures it; the HIP events of at_kernel_time also
 * hold the time the launch waits on the stream for free compute units).
 * Stamped by k_thr_ccl, k_ccl_border, k_boundary, k_extents, k_blob_small,
 * k_blob and k_decode; 0 launches for the other stages. */
int at_kernel_span(at_detector *d, double *avg_ms, long long *launches);

/* Work counts of the last collected batch: [0] frames, [1] boundary points,
 * [2] blob pairs, [3] points processed by the small-blob kernel, [4] by the
 * large-blob kernel, [5] fitted quads, [6] decoded candidates (pre-reconcile);
 * host time of this detector since creation, microseconds: [7] waiting in
 * at_collect for the GPU, [8] in the host tail (reconcile, sort, poses);
 * CCL: [9] local roots listed for the cross-tile merge (all frames), [10] their
 * maximum over the frames, [11] frames merged by the multi-workgroup fallback.
 * Returns the number of entries written. */
int at_batch_stats(at_detector *d, uint64_t *out, int cap);

/* Tag pose of each detection of the last collected batch (row A23): the
 * reference node's estimate_tag_pose(&info_, &pose) per detection
 * (apriltags_cuda_detector.cu:425-436; AprilTag 3.x orthogonal iteration with
 * the second-minimum check), computed on the GPU by the k_pose kernel when
 * at_config.tag_size > 0.  Entry i belongs to detection i of the frame (the
 * id-sorted order at_collect returned).  Returns the count or < 0. */
typedef struct {
  int32_t id;
  double R[9];     /* row-major rotation, tag -> camera */
  double t[3];     /* tag centre in the camera frame, metres (pose.t) */
  double err;      /* object-space error returned by estimate_tag_pose */
} at_pose;
int at_poses(at_detector *d, int frame, at_pose *out, int cap);

/* Detections of frame `frame` of the last collected batch again (the same records
 * at_collect wrote, id order), e.g. when its cap_per_frame was smaller than the
 * count it reported.  Returns the count or < 0. */
int at_detections(at_detector *d, int frame, at_detection *out, int cap);
/* Most detections one frame can yield (candidates before reconcile; the reference
 * keeps every detection, apriltag_detect.cu:618-663): a cap_per_frame this large
 * never truncates. */
int at_max_detections(void);

/* The node's per-frame tail over those poses (apriltags_cuda_detector.cu:425-462,
 * 595-599): robot = R_ext * t + t_ext (transformCameraToRobot), distance = |t|
 * in the camera frame, records sorted by ascending distance (stable).  Host
 * only; extr_R row-major 3x3 (NULL = identity), extr_t 3 (NULL = zero). */
typedef struct {
  int32_t id;
  double camera[3];   /* aprilTagInCameraFrame */
  double robot[3];    /* aprilTagInRobotFrame */
  double distance;
  double err;         /* pose_error */
} at_tag_detection;
int at_tag_detections(const at_pose *poses, int n, const double *extr_R, const double *extr_t,
                      at_tag_detection *out);

/* Shared game-piece preprocessing: the network input of
 * preprocess_image (src/game_piece_detection/src/game_piece_detection_node.cu:347-379:
 * cv::resize INTER_LINEAR to out_width x out_height, BGR->RGB for 3 channels or
 * BGR->GRAY for 1, x 1/255, NCHW float) computed on the GPU from the same BGR8
 * frames the detector reads.  at_gp_enable adds it to the launch sequence (every
 * later batch of AT_FMT_BGR8 frames); at_gp_tensor gives frame `frame`'s tensor of
 * the last batch in device memory (channels x out_height x out_width floats, valid
 * until the next batch); at_gp_copy copies it to the host.  AT_E_INVALID when the
 * last batch was neither BGR8 nor a colour-on MJPG batch.  at_gp_preprocess_device runs it standalone on one
 * device-resident BGR8 image on `stream` (a hipStream_t, NULL = default stream). */
int at_gp_enable(at_detector *d, int out_width, int out_height, int channels);
int at_gp_tensor(at_detector *d, int frame, const float **dev_ptr);
int at_gp_copy(at_detector *d, int frame, float *dst, size_t count);
int at_gp_preprocess_device(const uint8_t *bgr, int width, int height, float *out, int out_width, int out_height,
                            int channels, void *stream);

/* The game-piece node's output parse (game_piece_detection_node.cu:287-292 over
 * yolo_detection.h:53-209): what the reference does with the network's output tensor,
 * one frame being raw[(4 + C) * P] floats -- rows of P: x, y, w, h, score_0 .. score_{C-1}.
 *   parse_yolov11_output  per prediction the first class holding the maximum score above 0
 *                         (a NaN never wins; nothing above 0: class 0, confidence 0); the
 *                         prediction is dropped iff confidence < conf_thr (reference 0.25);
 *   apply_nms             candidates by descending confidence, equal ones by ascending
 *                         prediction index (the reference's std::sort leaves ties open;
 *                         this is what a stable sort gives); an unsuppressed candidate is
 *                         kept and suppresses every later one of its class with
 *                         iou > iou_thr (strict; reference 0.45), calculate_iou as written
 *                         there in float32 (std::max / std::min comparisons, IEEE division);
 *   scale_detections      x, w by (float)orig_w / (float)model_w, y, h likewise.
 * Boxes come out in NMS order (descending confidence).  The network itself is the user's
 * engine: it reads at_gp_tensor's pointer and leaves its output in device memory.
 *
 * at_gp_parse_host is that on the host (no device needed, no candidate cap): the CPU
 * reference, sharing the kernels' arithmetic (csrc/at_gp.h).  *n receives the number of
 * boxes kept; at most cap are written.
 *
 * at_gp_parse_device parses nframes tensors in device memory, frame_stride floats apart, on
 * the detector's stream, ordered after everything queued so far on `producer_stream` (a
 * hipStream_t of the same device, the stream the engine ran on; event + stream wait, no
 * host wait; NULL = the null stream), and returns when the boxes are in `out` (host memory,
 * frame f's at out + f * cap_per_frame).  n_per_frame[f] = boxes kept (at most cap_per_frame
 * written); status_per_frame[f] (may be NULL) = 0, or AT_E_CAPACITY for a frame with more
 * than AT_GP_MAX_CANDIDATES candidates, which yields zero boxes (never a silently different
 * answer; the other frames are unaffected; the reference reserves 1000, the deployed model
 * yields a few hundred).  orig_w / orig_h are the detector's geometry.  Nothing is
 * allocated per call: the buffers are allocated on the first call for max_batch frames.
 * AT_E_INVALID: a NULL, P < 1, C < 1, nframes outside 1..max_batch,
 * frame_stride < (4 + C) * P, a non-finite threshold, a model size < 1.
 *
 * at_gp_draw_boxes_device draws the boxes' outlines (detection_test.cpp:73-100: corners
 * truncated to int and clamped to the image, cv::rectangle of thickness 2 as four 2-px
 * segments, colour by cls % 6: green, orange, blue, yellow, magenta, cyan) onto a
 * device-resident BGR8 image of the detector's geometry, like at_draw_outlines_device;
 * pixel-identical to node/at_node.cpp's draw_boxes.  The reference's label text and filled
 * label background are not drawn (OpenCV's Hershey font is not carried here).
 * at_gp_parse_stats, the last at_gp_parse_device call: [0] candidates (sum over the frames),
 * [1] most candidates of one frame, [2] boxes kept, [3] the two kernels' time in
 * nanoseconds (HIP events; measured while at_set_profiling is on, 0 otherwise). */
typedef struct { float x, y, w, h, conf; int32_t cls; } at_gp_box;   /* 24 bytes */
#define AT_GP_MAX_CANDIDATES 4096
int at_gp_parse_host(const float *raw, int num_predictions, int num_classes,
                     float conf_thr, float iou_thr, int model_w, int model_h, int orig_w, int orig_h,
                     at_gp_box *out, int cap, int *n);
int at_gp_parse_device(at_detector *d, const float *d_raw, size_t frame_stride, int nframes,
                       int num_predictions, int num_classes, float conf_thr, float iou_thr,
                       int model_w, int model_h, void *producer_stream,
                       at_gp_box *out, int cap_per_frame, int *n_per_frame, int *status_per_frame);
int at_gp_draw_boxes_device(at_detector *d, const at_gp_box *boxes, int n, uint8_t *bgr);
int at_gp_parse_stats(at_detector *d, uint64_t *out, int cap);
/* The boxes on the frame a host-fed batch staged in HBM, for a node without device memory of
 * its own: at_annotate_staged / at_annotate_jpeg with boxes in place of tag outlines (same
 * gating: AT_E_INVALID unless the last batch was host BGR8 frames or a colour-on MJPG batch and
 * `frame` one of its frames; the staged image is consumed; same capacity rule for the JPEG).
 * at_gp_copy_raw copies `count` floats of a tensor in device memory to the host on the
 * detector's stream (e.g. the tensor of an AT_E_CAPACITY frame, for at_gp_parse_host). */
int at_gp_annotate_staged(at_detector *d, int frame, const at_gp_box *boxes, int n, uint8_t *bgr_out);
int at_gp_annotate_jpeg(at_detector *d, int frame, const at_gp_box *boxes, int n, int quality, int sampling,
                        uint8_t *out, size_t cap, size_t *len);
int at_gp_copy_raw(at_detector *d, const float *d_raw, float *dst, size_t count);

/* The annotated image on the GPU: the node's outlined frame
 * (apriltag_utils.cu:54-79, drawn on the host with cv::line / cv::putText by
 * apriltags_cuda_detector.cu:514-518) drawn onto a device-resident BGR8 image of
 * the detector's geometry (width x height x 3, row-major): per detection the four
 * sides (0-1 green, 0-3 red, 1-2 / 2-3 blue; corners truncated to int as
 * cv::Point does) and the id centred on c, 2-px segments.  Pixel-identical to
 * node/at_node.cpp's draw_detection_outlines (its digit glyphs, not OpenCV's
 * Hershey font).  `dets` as at_collect returned them (host memory).  Runs on the
 * detector's stream and returns when the image is drawn. */
int at_draw_outlines_device(at_detector *d, const at_detection *dets, int n, uint8_t *bgr);

/* The node's published image for a host-fed BGR8 frame without a host copy and
 * redraw: draws those outlines onto frame `frame` of the last batch where
 * at_detect / at_detect_batch staged it in HBM, and copies the annotated image
 * (width x height x 3) to `bgr_out` in host memory.  AT_E_INVALID unless the last
 * batch was host BGR8 frames or a colour-on MJPG batch (then the decoded image is what
 * is drawn on).  The staged copy is consumed (overwritten). */
int at_annotate_staged(at_detector *d, int frame, const at_detection *dets, int n, uint8_t *bgr_out);

/* The annotated image as a finished JPEG, encoded on the GPU: what the node's consumers
 * read is the compressed topic (image_transport, the viewer's cv::imencode), so the image
 * need not cross the link at 3 B per pixel to be encoded on a host core.
 *
 * The stream: baseline SOF0, 8 bit, YCbCr, one interleaved scan; sampling AT_JPEG_420 (what
 * cv::imencode writes), AT_JPEG_422 or AT_JPEG_444; libjpeg's quality rule, quality 1..100
 * (OpenCV's default is 95); the Annex K Huffman tables; one restart interval per MCU row
 * (DRI = MCUs per row, RSTm between rows).  Header: SOI, a JFIF APP0, DQT, DQT, SOF0, four
 * DHT, DRI, SOS.  Every non-APPn segment and the entropy-coded data equal byte for byte
 * what libjpeg(-turbo) writes for the same image with its integer "slow" DCT and
 * restart_in_rows = 1 (Pillow: save(..., restart_marker_rows=1)).
 *
 * at_encode_jpeg_device encodes a device-resident BGR8 image of the detector's geometry
 * (width x height x 3, row-major, 8-byte aligned) on the detector's stream into host memory
 * (the counterpart of at_draw_outlines_device); it returns when the bytes are in `out`.
 * at_annotate_jpeg is at_annotate_staged with that encode in place of the raw copy: same
 * gating (AT_E_INVALID unless the last batch was host BGR8 frames or a colour-on MJPG batch
 * and `frame` one of its frames), the staged image is consumed, and only the stream's bytes
 * cross the link.  *len receives the stream's size.  If it exceeds cap the result is
 * AT_E_CAPACITY, *len is the size needed and nothing is written to `out`;
 * at_jpeg_max_bytes(width, height, sampling) is a capacity no image can exceed (0 for a
 * geometry the encoder does not take: multiples of 8 up to 65528).  quality outside 1..100
 * or an unknown sampling: AT_E_INVALID.  The device buffers are allocated on the first call
 * at the worst case of the geometry and kept.  `out` page-locked (at_host_alloc) is copied
 * into by DMA.
 * at_jpeg_stats, the last encode: [0] bytes of the stream, [1] the time of the encode
 * kernels in nanoseconds (HIP events; measured while at_set_profiling is on, 0 otherwise).
 * at_jpeg_encode_host is the same encoder on the host (no device needed; any width and
 * height that are multiples of 8): the CPU reference, sharing the kernels' arithmetic. */
enum { AT_JPEG_420 = 0, AT_JPEG_422 = 1, AT_JPEG_444 = 2 };
int at_encode_jpeg_device(at_detector *d, const uint8_t *bgr, int quality, int sampling, uint8_t *out, size_t cap,
                          size_t *len);
int at_annotate_jpeg(at_detector *d, int frame, const at_detection *dets, int n, int quality, int sampling,
                     uint8_t *out, size_t cap, size_t *len);
size_t at_jpeg_max_bytes(int width, int height, int sampling);
int at_jpeg_stats(at_detector *d, uint64_t *out, int cap);
int at_jpeg_encode_host(const uint8_t *bgr, int width, int height, int quality, int sampling, uint8_t *out,
                        size_t cap, size_t *len);

/* The preview stream: the annotated image small enough for a robot's radio link (the
 * seasocks viewer's websocket, the bag recording's /compressed topic), for a frame of ANY
 * input format -- YUYV and mono8 cameras and the luma-only MJPG route have no annotated
 * image otherwise.
 *
 * Geometry (at_preview_size, host only): scale s is an integer 1..8; pw = (width / s) & ~7,
 * ph = (height / s) & ~7 (the encoder's multiples of 8); the crop of pw * s x ph * s source
 * pixels is centred, ox = (width - pw * s) / 2, oy likewise.  pw < 8 or ph < 8 (or s outside
 * 1..8): AT_E_INVALID.  s = 1 is "convert only": the full-size annotated image.
 *
 * Image: every source pixel is converted to BGR8 (GRAY8: B = G = R = Y; YUYV: pixel x takes
 * the U and V of its pair, 20-bit fixed-point BT.601 limited range:
 *   y = max(0, Y - 16) * 1220542,  R = sat8((y + (1 << 19) + 1673527 (V - 128)) >> 20),
 *   G = sat8((y + (1 << 19) - 852492 (V - 128) - 409993 (U - 128)) >> 20),
 *   B = sat8((y + (1 << 19) + 2116026 (U - 128)) >> 20) -- OpenCV's COLOR_YUV2BGR_YUY2 as
 * remembered; equality with cv::cvtColor is not pinned by a test), then averaged per channel
 * over its s x s box, (sum + s * s / 2) / (s * s), integers only.  The records are mapped
 * before anything is drawn -- corners and centre (p - o) / s in double, a box x' = (x - ox) / s,
 * w' = w / s in float -- and drawn at pw x ph like the full-size image: boxes first, tag
 * outlines on top, lines 2 px, id glyphs at their fixed size.
 *
 * at_preview_bgr / at_preview_jpeg take frame `frame` of the last batch where it was staged
 * in HBM: AT_E_INVALID unless that batch was host-fed (at_detect*, at_enqueue_host,
 * at_enqueue_mjpg with or without colour; a luma-only MJPG batch gives the decoded gray
 * plane) and `frame` one of its frames.  A pending batch is waited for.  The staged frame is
 * only read (unlike at_annotate_staged).  at_preview_jpeg_device takes one device-resident
 * frame of the detector's geometry in `fmt` (at_enqueue_device batches): NULL or not 8-byte
 * aligned is AT_E_INVALID.  The preview image lives in a buffer allocated on the first call.
 *
 * The JPEG is at_encode_jpeg_device's stream at pw x ph.  max_bytes == 0: one encode at
 * `quality`.  max_bytes > 0, the per-frame byte budget: encode at `quality`; if that is
 * larger, bisect on [1, quality - 1] (mid = (lo + hi + 1) / 2; lo = mid if it fits, else
 * hi = mid - 1; until lo == hi) and return the encode at lo -- this rule, not "the best
 * quality", is the contract, since JPEG size is not strictly monotonic in quality.  At most
 * 2 + ceil(log2(quality - 1)) encodes: 8 from quality 50, 9 from 100.  If quality 1 does not
 * fit: AT_E_CAPACITY, *len its size, *quality_used = 1, nothing written.  A stream larger than
 * cap: AT_E_CAPACITY with *len the size needed, as at_annotate_jpeg.  *quality_used (may be
 * NULL) is the quality of the stream returned.
 *
 * at_preview_host / at_preview_jpeg_host: the same on the CPU (no device; any w x h whose
 * preview is at least 8 x 8, w even for YUYV; cap >= pw * ph * 3) through the same arithmetic,
 * mapping and search -- the reference of the device path, bit for bit.
 * at_preview_stats, the last preview call: [0] bytes returned, [1] quality used, [2] encodes
 * run, [3] pw, [4] ph, [5] the kernels' time in nanoseconds (HIP events; while
 * at_set_profiling is on, 0 otherwise).
 * All calls are synchronous, on the detector's stream, outside the captured graphs. */
int at_preview_size(int width, int height, int scale, int *pw, int *ph, int *ox, int *oy);
int at_preview_bgr(at_detector *d, int frame, int scale, const at_detection *dets, int n, const at_gp_box *boxes,
                   int nb, uint8_t *bgr_out);
int at_preview_jpeg(at_detector *d, int frame, int scale, const at_detection *dets, int n, const at_gp_box *boxes,
                    int nb, int quality, int sampling, size_t max_bytes, uint8_t *out, size_t cap, size_t *len,
                    int *quality_used);
int at_preview_jpeg_device(at_detector *d, const void *d_frame, at_pixfmt fmt, int scale, const at_detection *dets,
                           int n, const at_gp_box *boxes, int nb, int quality, int sampling, size_t max_bytes,
                           uint8_t *out, size_t cap, size_t *len, int *quality_used);
int at_preview_host(const uint8_t *frame, at_pixfmt fmt, int w, int h, int scale, const at_detection *dets, int n,
                    const at_gp_box *boxes, int nb, uint8_t *bgr_out, size_t cap);
int at_preview_jpeg_host(const uint8_t *frame, at_pixfmt fmt, int w, int h, int scale, const at_detection *dets,
                         int n, const at_gp_box *boxes, int nb, int quality, int sampling, size_t max_bytes,
                         uint8_t *out, size_t cap, size_t *len, int *quality_used);
int at_preview_stats(at_detector *d, uint64_t *out, int cap);

/* Field pose: one camera pose per frame from every tag of a known layout in it.
 *
 * k_pose gives each tag's own pose (four coplanar corners, the two-minimum ambiguity).  With
 * a field layout set -- where each tag stands on the field, x_field = R x_tag + t, the tag
 * frame being at_pose's: corners at (-+s/2, +-s/2, 0) in at_detection.p order, s = tag_size
 * -- one more kernel (k_field, after k_pose in the launch sequence, like at_gp_enable's; gone
 * again when the layout is cleared) solves per frame for the one camera pose that explains
 * the corners of all its layout tags, and leaves it in mapped host memory: at_collect copies
 * nothing more.
 *
 * Per frame:
 *   select  the candidates (before reconcile) with an id of the layout and hamming <=
 *           max_hamming; per id the lowest hamming, then the greatest decision_margin, then
 *           the lowest candidate slot; the AT_FIELD_MAX_TAGS lowest ids;
 *   points  each tag's corners in the field frame against at_detection.p through fx, fy,
 *           cx, cy (p as k_pose reads it: no further undistortion);
 *   start   each used tag's own pose as a camera pose, R_j = pose_R R_tag^T,
 *           t_j = pose_t - R_j t_tag; the one with the least summed squared reprojection
 *           error over all points (a point at Z <= 0: infinite; ties: the lower id);
 *   refine  12 Levenberg-Marquardt iterations on the pixel residuals (6 parameters, rotation
 *           update left-multiplied from q = (1, w / 2) normalised, damping lambda diag(J^T J)
 *           from 1e-3, / 10 (floor 1e-9) on an accepted step, x 10 on a rejected one; a step
 *           is accepted only if the cost falls and every Z stays positive).
 * A frame without a layout tag (or whose tags' poses all put a point behind the camera) has
 * n_tags = 0 and the rest zero.
 *
 * at_set_field_layout: n = 0 clears.  AT_E_INVALID: at_config.tag_size == 0, an id outside
 * [0, 1024), an id twice, an R with |R R^T - I| above 1e-6 or det < 0, max_hamming < 0, a batch
 * not yet collected.  It takes effect from the next enqueued batch.
 * at_field_poses: one record per frame of the last collected batch (all n_tags = 0 if it ran
 * without a layout); returns the frame count, writes at most cap.
 * at_field_pose_host: the same solve on the CPU for one frame's at_detections / at_poses
 * arrays (the CPU reference: it shares the kernel's arithmetic and takes the same
 * accept / reject decisions); checks `tags` like at_set_field_layout.
 * at_robot_in_field (host only): the robot's pose in the field, field_T_cam (robot_T_cam)^-1
 * with the camera -> robot extrinsics of at_tag_detections (NULL = identity / zero):
 * x_field = R_out x_robot + t_out.  AT_E_INVALID for a record with n_tags = 0.
 * at_field_stats, the last collected batch: [0] frames solved, [1] tags used, [2] candidates
 * dropped by the 16-tag cap, [3] rejected LM steps, [4] k_field's time in nanoseconds (HIP
 * events; while at_set_profiling is on, 0 otherwise). */
typedef struct { int32_t id; double R[9]; double t[3]; } at_field_tag;
#define AT_FIELD_MAX_TAGS 16
typedef struct {
  int32_t n_tags;                   /* tags used; 0 = no layout tag in this frame (rest zeroed) */
  int32_t ids[AT_FIELD_MAX_TAGS];   /* ascending */
  double R[9]; double t[3];         /* x_cam = R x_field + t, row-major, like at_pose */
  double rms_px;                    /* reprojection RMS over the 4*n_tags corners */
  int32_t steps_taken;              /* accepted LM steps */
} at_field_pose;
int at_set_field_layout(at_detector *d, const at_field_tag *tags, int n, int max_hamming);
int at_field_poses(at_detector *d, at_field_pose *out, int cap);
int at_field_pose_host(const at_detection *dets, const at_pose *poses, int n, const at_field_tag *tags, int ntags,
                       int max_hamming, const at_camera *cam, double tag_size, at_field_pose *out);
int at_robot_in_field(const at_field_pose *fp, const double *extr_R, const double *extr_t, double *R_out, double *t_out);
int at_field_stats(at_detector *d, uint64_t *out, int cap);

/* Ideal corners: the lens distortion undone before every pose solve (opt-in, off by default).
 *
 * The pose solves project through a pinhole, which is exact against *ideal* pixels: the raw ones
 * mapped through the inverse of the forward model (k1, k2, p1, p2, k3 of at_camera, as
 * at_camcal solves them).  With the mode on, the head of the pose stage maps each candidate's
 * four corners (eight Newton steps with the analytic Jacobian, no early exit), recomputes H from
 * them (homography_compute2's elimination) and c as the image of (0, 0); the tag pose, the field
 * pose and the rig pose (per member; members with the mode on and off may be mixed) are computed
 * from those.  No launch is added.  at_detections, at_collect, the annotated image, the preview
 * and the camera calibration stay on raw corners.
 *
 * A pixel is not invertible when the Jacobian's determinant is not > 0 at an iterate or at the
 * result (the model folds over: lenses with a large negative k3, near the image corners), or the
 * result's forward image is not within 1e-6 px of it on each axis; NaN and infinity are not.  A
 * detection with such a corner has an ideal record that is its raw record with id = -1: the
 * field, rig, calibration and mapping selections pass it over; its own at_pose comes from its raw
 * corners.  With all five coefficients zero the ideal record is a copy of the raw one.
 *
 * at_set_undistort: from the next enqueued batch; AT_E_INVALID for a NULL detector, a batch not
 * yet collected, at_config.tag_size not positive.
 * at_ideal_detections: like at_detections (same order and count), with H, c, p ideal and id = -1
 * where not invertible; AT_E_INVALID when the last batch ran with the mode off.
 * at_ideal_detections_host: the CPU twin on at_detections' records, bit-equal; returns n.
 * at_undistort_points: n pixels (u, v pairs) through the same inverse on the detector's stream
 * (k_und_points; for pixels that are no tag corners, such as a game piece's box centre); ok[i] = 0
 * and out = the raw pixel where pixel i is not invertible.  Needs no mode; returns n.
 * at_undistort_points_host: the CPU twin, bit-equal.
 * at_undistort_stats, the last collected batch: [0] detections made ideal, [1] detections not
 * invertible (both 0 with the mode off). */
int at_set_undistort(at_detector *d, int on);
int at_ideal_detections(at_detector *d, int frame, at_detection *out, int cap);
int at_ideal_detections_host(const at_camera *cam, const at_detection *dets, int n, at_detection *out);
int at_undistort_points(at_detector *d, const double *xy, int n, double *out_xy, uint8_t *ok);
int at_undistort_points_host(const at_camera *cam, const double *xy, int n, double *out_xy, uint8_t *ok);
int at_undistort_stats(at_detector *d, uint64_t *out, int cap);

/* Rig pose: one robot pose per instant from the layout tags of every camera, with its covariance.
 *
 * A rig is 1..AT_RIG_MAX_CAMS detectors of one process on one device, each with its own
 * at_camera and its extrinsics x_robot = R x_cam + t (at_tag_detections' convention); frame f of
 * every member's last batch is instant f.  The unknown is the robot in the field,
 * x_field = R x_robot + t.  One kernel (k_rig, one workgroup per instant, one wave per camera)
 * on the rig's own stream; it is part of no member's launch sequence, reads the members'
 * candidates and writes nothing of theirs.
 *
 * Per instant:
 *   select  per camera as the field pose does (at most AT_FIELD_MAX_TAGS tags each);
 *   points  a corner X of the field projects as Q = R^T (X - t), P = E_R^T (Q - E_t),
 *           u = fx Px / Pz + cx, v = fy Py / Pz + cy against at_detection.p; Pz <= 0: infinite cost;
 *   start   each selected tag's own pose as a robot pose,
 *           field_T_tag (cam_T_tag)^-1 (robot_T_cam)^-1; the one with the least summed squared
 *           reprojection error over all corners of all cameras (ties: the lower camera, then
 *           the lower id), its rotation made orthonormal;
 *   refine  12 Levenberg-Marquardt iterations as the field pose's, parameters (w, dt) with
 *           R' = R dR(w) (w in the robot frame, dR from q = (1, w / 2) normalised) and
 *           t' = t + dt (field frame);
 *   cov     sigma^2 (J^T J)^-1 at the final pose, sigma^2 = cost / (8 n_tags - 6), row-major
 *           6 x 6 in the order (w_x, w_y, w_z, t_x, t_y, t_z): cov[21], cov[28], cov[35] are the
 *           field-frame position variances, cov[14] the variance of the turn about the robot's
 *           z.  cov_valid = 0 (and zeros) when J^T J has no Cholesky factor.
 * An instant without a layout tag in any camera has n_tags = 0 and the rest zero.
 *
 * at_rig_create: AT_E_INVALID for n_cams outside 1..AT_RIG_MAX_CAMS, a NULL member, a member
 * twice, members on different devices, at_config.tag_size 0 or differing between members, a
 * layout at_set_field_layout would refuse (n_tags = 0 included), max_hamming < 0.  The members
 * need no field layout of their own and must outlive the rig.
 * at_rig_solve: the members' last batches (pending or collected; it waits for them on its own
 * stream and does not collect them) must have one frame count, else AT_E_INVALID, as when a
 * member has run none.  Returns the number of instants, writes at most cap records.
 * at_rig_stats, the last solve: [0] instants solved, [1] tags used, [2] candidates dropped by the
 * per-camera cap, [3] rejected LM steps, [4] k_rig's time in nanoseconds (HIP events; while
 * at_set_profiling is on for a member, 0 otherwise).
 * at_rig_pose_host: the same solve on the CPU for one instant (the CPU reference: the kernel's
 * arithmetic in the kernel's order, bit-equal records). */
#define AT_RIG_MAX_CAMS 8
typedef struct { double R[9]; double t[3]; } at_rig_extrinsics;     /* x_robot = R x_cam + t */
typedef struct {
  int32_t n_tags;                                      /* total over the cameras; 0: rest zeroed */
  int32_t n_cams_used;                                 /* cameras with at least one tag */
  int32_t tags_per_cam[AT_RIG_MAX_CAMS];
  int32_t ids[AT_RIG_MAX_CAMS][AT_FIELD_MAX_TAGS];     /* per camera, ascending */
  double R[9]; double t[3];                            /* x_field = R x_robot + t, row-major */
  double cov[36];
  double rms_px;                                       /* reprojection RMS over the 4*n_tags corners */
  int32_t cov_valid;
  int32_t steps_taken;                                 /* accepted LM steps */
  int32_t rejected;                                    /* LM steps not taken */
  int32_t dropped;                                     /* eligible candidates beyond a camera's 16 lowest ids */
} at_rig_pose;
typedef struct {
  const at_detection *dets; const at_pose *poses; int32_t n;   /* one frame's at_detections / at_poses */
  const at_camera *cam;
  at_rig_extrinsics extr;
} at_rig_host_cam;
typedef struct at_rig at_rig;
int at_rig_create(at_detector *const *dets, const at_rig_extrinsics *extr, int n_cams,
                  const at_field_tag *tags, int n_tags, int max_hamming, at_rig **out);
int at_rig_solve(at_rig *r, at_rig_pose *out, int cap);
int at_rig_stats(at_rig *r, uint64_t *out, int cap);
void at_rig_destroy(at_rig *r);
int at_rig_pose_host(const at_rig_host_cam *cams, int n_cams, const at_field_tag *tags, int n_tags,
                     int max_hamming, double tag_size, at_rig_pose *out);

/* Robust rig pose: the rig pose with Huber weights on the corners and rejection of bad tags, so
 * that one wrong tag (a layout tag bumped on the field, a false decode, a corner dragged by glare)
 * does not poison the fused pose.  One kernel (k_rig_robust, launched as k_rig is: one workgroup
 * per instant, one wave per camera, the rig's own stream); at_rig_solve and at_rig_stats are not
 * touched by it, and a plain solve after a robust one returns what it returned before.
 *
 * Per instant, with s = ru^2 + rv^2 of a corner and k = huber_px:
 *   cost    rho = s while s <= k^2, else 2 k sqrt(s) - k^2, weight w = 1 resp. k / sqrt(s);
 *   start   as the rig pose, by the least summed rho;
 *   fit     the rig pose's 12 LM iterations on the summed rho, each corner's rows of the normal
 *           equations times its w at the linearisation point;
 *   reject  at most max_rounds times: a kept tag whose four corners have (s0 + s1) + (s2 + s3) >
 *           4 reject_px^2 at the current pose is a candidate; none: done; dropping them all would
 *           leave fewer than min_keep tags (counted per camera view): nothing is dropped,
 *           starved = 1, done; else all are dropped and the fit runs again from the current pose;
 *   result  rms_px = sqrt(sum s / (4 n_kept)) over the kept corners, cov = sum w s / (8 n_kept - 6)
 *           times (J^T W J)^-1, tag_rms_px of every selected tag, dropped ones included.
 * In the record n_tags, n_cams_used, tags_per_cam and ids are the selection, as at_rig_solve gives
 * them; steps_taken and rejected are totals over all fits.  In the info: rounds is the number of
 * rounds that dropped tags (fits run after the first), rejected_mask[c] bit j is set when
 * ids[c][j] of the record was dropped, huber_cost the final summed rho, n_downweighted the kept
 * corners beyond huber_px at the final pose.  With huber_px = reject_px = +infinity the record is
 * at_rig_solve's bit for bit.
 * Limits: a tag is tested under a pose it helped to fit.  A small displacement among few tags is
 * absorbed by the pose and is not detected (2 cm in a one-camera view of three tags is not), and
 * when most tags are wrong the fit follows them and drops the good ones.
 *
 * AT_E_INVALID for a NULL config or info, huber_px or reject_px not > 0 (NaN included; +infinity
 * is valid), max_rounds outside 0..3, min_keep < 1, and whatever at_rig_solve / at_rig_pose_host
 * refuse.  at_rig_solve_robust writes at most cap records and infos and returns the number of
 * instants.  at_rig_robust_stats, the last robust solve: [0] instants solved, [1] tags dropped,
 * [2] rounds run, [3] starved instants, [4] k_rig_robust's time in nanoseconds (as at_rig_stats).
 * at_rig_pose_robust_host: the same solve on the CPU for one instant, bit-equal record and info. */
typedef struct { double huber_px, reject_px; int32_t max_rounds, min_keep; } at_rig_robust_config; /* 24 B */
typedef struct {
  int32_t n_kept, n_rejected, rounds, starved;
  uint32_t rejected_mask[AT_RIG_MAX_CAMS];                 /* bit j: ids[cam][j] of the record was dropped */
  double tag_rms_px[AT_RIG_MAX_CAMS][AT_FIELD_MAX_TAGS];   /* 0 beyond tags_per_cam */
  double huber_cost;
  int32_t n_downweighted, pad;                             /* kept corners beyond huber_px at the end */
} at_rig_robust_info;
int at_rig_solve_robust(at_rig *r, const at_rig_robust_config *cfg, at_rig_pose *out, at_rig_robust_info *info,
                        int cap);
int at_rig_pose_robust_host(const at_rig_host_cam *cams, int n_cams, const at_field_tag *tags, int n_tags,
                            int max_hamming, double tag_size, const at_rig_robust_config *cfg, at_rig_pose *out,
                            at_rig_robust_info *info);
int at_rig_robust_stats(at_rig *r, uint64_t *out, int cap);

/* Rig calibration: the cameras' extrinsics from recorded instants (bundle adjustment).
 *
 * Unknowns: the robot's field pose at every stored instant and, per camera, the rotation
 * (free_rot) and / or translation (free_trans) of its extrinsics x_robot = R x_cam + t.  Cost: the
 * summed squared reprojection error in pixels of every selected layout-tag corner of every camera
 * at every instant, projected as the rig pose does.  Parameters: per instant (w, dt) as the rig
 * pose; per camera (we, de) with R' = R dR(we), t' = t + de.  16 Levenberg-Marquardt iterations on
 * the whole problem through the Schur complement of the pose blocks, lambda from 1e-3, / 10
 * (floor 1e-9) on an accepted step (the total cost fell), x 10 on a rejected one; a reduced system
 * without a Cholesky factor is a rejected iteration.  Every instant starts from the rig pose
 * under the initial extrinsics; one that gets none (n_tags = 0) is skipped.
 *
 * at_rigcal_create: AT_E_INVALID for n_cams outside 2..AT_RIG_MAX_CAMS, no camera with both
 * flags 0 (the robot frame would float), no flag set at all, a layout at_set_field_layout would
 * refuse, max_hamming < 0, tag_size not positive, an R that is no rotation (the layout's bound).
 * at_rigcal_add: one instant, frames[c] the at_detections / at_poses arrays of camera c's frame;
 * per camera the rig pose's selection is stored (at most AT_FIELD_MAX_TAGS tags: id, corners, the
 * tag's own pose).  Returns 1 if stored, 0 if fewer than two cameras had a selected tag (such an
 * instant constrains no extrinsic), AT_E_CAPACITY beyond AT_RIGCAL_MAX_INSTANTS.
 * at_rigcal_solve: the solve on the GPU (kernels k_cal_*, on a stream of the calibrator's own; one
 * synchronisation, at the end).  at_rigcal_solve_host: the same on the CPU, the kernels'
 * arithmetic in the kernels' order: bit-equal records.  Both AT_E_INVALID without a stored
 * instant.  cov is sigma^2 times camera c's 6 x 6 block of the inverse of the undamped reduced
 * matrix at the final state, order (we, de), sigma^2 = cost / (2 corners - 6 instants_used - free
 * parameters); rows and columns of parameters that are not free are zero; cov_valid = 0 (and
 * zeros) without a factor or with a denominator that is not positive.
 * at_rigcal_instants: per stored instant of the last solve, its final robot pose and RMS
 * (used = 0: skipped, rest zero); returns the count, writes at most cap.
 * at_rigcal_stats, the last solve: [0] instants used, [1] skipped, [2] accepted steps,
 * [3] rejected steps, [4] the kernels' time in nanoseconds (HIP events around the sequence of the
 * last at_rigcal_solve while at_rigcal_set_profiling is on, 0 otherwise). */
#define AT_RIGCAL_MAX_INSTANTS 4096
typedef struct {
  at_camera cam;
  at_rig_extrinsics extr;              /* the initial extrinsics */
  int32_t free_rot, free_trans;
} at_rigcal_camera;
typedef struct { const at_detection *dets; const at_pose *poses; int32_t n; } at_rigcal_frame;
typedef struct {
  double R[9]; double t[3];            /* x_robot = R x_cam + t */
  double cov[36];
} at_rigcal_camera_result;
typedef struct {
  double rms_before, rms_after;        /* pixels, over the corners of the instants used */
  int32_t instants_used, instants_skipped;
  int32_t accepted, rejected;
  int32_t cov_valid, n_cams;
  at_rigcal_camera_result cams[AT_RIG_MAX_CAMS];
} at_rigcal_result;
typedef struct {
  double R[9]; double t[3];            /* x_field = R x_robot + t */
  double rms_px;
  int32_t n_tags, used;
} at_rigcal_instant;
typedef struct at_rigcal at_rigcal;
int at_rigcal_create(const at_rigcal_camera *cams, int n_cams, const at_field_tag *tags, int n_tags,
                     int max_hamming, double tag_size, at_rigcal **out);
int at_rigcal_add(at_rigcal *c, const at_rigcal_frame *frames);
int at_rigcal_count(const at_rigcal *c);
int at_rigcal_clear(at_rigcal *c);
int at_rigcal_solve(at_rigcal *c, at_rigcal_result *out);
int at_rigcal_solve_host(at_rigcal *c, at_rigcal_result *out);
int at_rigcal_instants(const at_rigcal *c, at_rigcal_instant *out, int cap);
int at_rigcal_set_profiling(at_rigcal *c, int on);
int at_rigcal_stats(const at_rigcal *c, uint64_t *out, int cap);
void at_rigcal_destroy(at_rigcal *c);

/* Rig track: the robot's field pose over a sliding window of instants linked by odometry.
 *
 * A fixed-lag smoother.  The window is the last `window` pushed instants, oldest dropped first,
 * always one connected chain.  An instant holds, per camera, the rig pose's selection of layout
 * tags (what at_rigcal_add stores), a time stamp (passed through) and the odometry since the
 * previous instant: the robot now in the previous instant's robot frame, x_prev = R x_now + t, with
 * standard deviations sigma_rot (radians) and sigma_trans (metres).  An instant in which no camera
 * has a layout tag is stored too: its odometry alone holds it.
 * Unknowns: x_field = R_k x_robot + t_k at every instant, parameters (w, dt) as the rig pose.  Cost:
 * every selected corner's pixel residual / sigma_px (projected as the rig pose does; Pz <= 0 costs
 * infinity), and for k >= 1, with E = R_m^T R_{k-1}^T R_k, the rotation residual
 * 1/2 (E[7] - E[5], E[2] - E[6], E[3] - E[1]) / sigma_rot and the translation residual
 * (R_{k-1}^T (t_k - t_{k-1}) - t_m) / sigma_trans.
 * Start, a pure function of the window: an instant with tags starts from the rig pose over its
 * stored tags; one without from its predecessor's start composed with its odometry; leading
 * tagless instants backwards from the first instant that has a start.
 * `iters` Levenberg-Marquardt iterations, lambda from 1e-3, / 10 (floor 1e-9) on an accepted step
 * (the total cost fell and every Pz stayed positive), x 10 on a rejected one; the block-tridiagonal
 * normal equations are solved by block Cholesky in ascending instants, and a pivot that is not
 * positive is a rejected iteration.  cov is the inverse of the latest instant's last Schur block of
 * the undamped system at the final state, order (w, t), not rescaled; cov_valid = 0 (and zeros)
 * without a factor.
 *
 * at_rigtrack_create: AT_E_INVALID for a NULL, n_cams outside 1..AT_RIG_MAX_CAMS, a layout
 * at_set_field_layout would refuse, max_hamming < 0, tag_size or sigma_px not positive and finite,
 * an R that is no rotation, window outside 2..AT_RIGTRACK_MAX_WINDOW, iters outside 1..16.
 * at_rigtrack_push: one instant, frames[c] as at_rigcal_add (at most AT_FIELD_MAX_TAGS tags per
 * camera are kept).  odom = NULL: the first instant of a chain; with instants stored the window is
 * emptied first (odometry was lost).  AT_E_INVALID for a NULL, a frame with n < 0 or n > 0 and a
 * NULL array, an odom whose R is no rotation, whose t is not finite or whose sigmas are not positive
 * and finite; nothing changes then.  Returns the window's count.
 * at_rigtrack_solve: the solve on the GPU (kernels k_trk_*, on a stream of the tracker's own; one
 * synchronisation, at the end).  at_rigtrack_solve_host: the same on the CPU, the kernels'
 * arithmetic in the kernels' order: bit-equal records.  Neither changes what a later solve gives.
 * Both AT_E_INVALID for an empty window or one in which no instant has a start.
 * at_rigtrack_instants: per instant of the last solve, oldest first; returns the count, writes at
 * most cap.  rms_px = 0 for n_tags = 0.
 * at_rigtrack_stats, the last solve: [0] window size, [1] tags used, [2] accepted steps,
 * [3] rejected steps, then the kernels' time in nanoseconds from HIP events while
 * at_rigtrack_set_profiling is on (0 otherwise; a profiled solve records an event pair per launch):
 * [4] all, [5] k_trk_start and k_trk_fill, [6] k_trk_accum, [7] k_trk_solve. */
#define AT_RIGTRACK_MAX_WINDOW 64
typedef struct {
  at_camera cam;
  at_rig_extrinsics extr;
} at_rigtrack_camera;
typedef struct {
  double R[9]; double t[3];            /* x_prev = R x_now + t */
  double sigma_rot, sigma_trans;
} at_rigtrack_odom;
typedef struct {
  int32_t n, with_tags;                /* instants in the window, of them with a start of their own */
  int32_t accepted, rejected;
  double cost_before, cost_after;      /* the whole cost, sigmas applied */
  double rms_before, rms_after;        /* pixels, over the corners */
  double R[9]; double t[3];            /* the latest instant: x_field = R x_robot + t */
  double cov[36];
  double stamp;
  int32_t cov_valid, pad;
} at_rigtrack_result;
typedef struct {
  double R[9]; double t[3];
  double stamp;
  double rms_px;
  int32_t n_tags, pad;
} at_rigtrack_instant;
typedef struct at_rigtrack at_rigtrack;
int at_rigtrack_create(const at_rigtrack_camera *cams, int n_cams, const at_field_tag *tags, int n_tags,
                       int max_hamming, double tag_size, double sigma_px, int window, int iters,
                       at_rigtrack **out);
int at_rigtrack_push(at_rigtrack *t, double stamp, const at_rigcal_frame *frames, const at_rigtrack_odom *odom);
int at_rigtrack_count(const at_rigtrack *t);
int at_rigtrack_clear(at_rigtrack *t);
int at_rigtrack_solve(at_rigtrack *t, at_rigtrack_result *out);
int at_rigtrack_solve_host(at_rigtrack *t, at_rigtrack_result *out);
int at_rigtrack_instants(const at_rigtrack *t, at_rigtrack_instant *out, int cap);
int at_rigtrack_set_profiling(at_rigtrack *t, int on);
int at_rigtrack_stats(const at_rigtrack *t, uint64_t *out, int cap);
void at_rigtrack_destroy(at_rigtrack *t);

/* Camera calibration: the intrinsics and distortion of one camera from views of a tag board.
 *
 * A board is an at_field_tag array: each tag's pose in the board frame, any rigid arrangement.
 * Unknowns: the board's pose in every stored view (x_cam = R x_board + t) and the entries of
 * (fx, fy, cx, cy, k1, k2, p1, p2, k3) that free_mask selects (AT_CAMCAL_FX .. AT_CAMCAL_K3);
 * free_mask = 0 fits the view poses only, which scores an existing calibration.  Cost: the summed
 * squared error in pixels of every stored corner against at_detection.p under the detector's
 * forward model (x = Px/Pz, y = Py/Pz, r2 = x x + y y, lin = 1 + k1 r2 + k2 r2^2 + k3 r2^3,
 * x'' = x lin + 2 p1 x y + p2 (r2 + 2 x x), y'' = y lin + p1 (r2 + 2 y y) + 2 p2 x y, u = fx x'' + cx,
 * v = fy y'' + cy); a corner at Pz <= 0 costs infinity.  Record the views with the detector's
 * distortion set to zero, so that p is the raw pixel.
 * 30 Levenberg-Marquardt iterations on the whole problem through the Schur complement of the
 * views' 6 x 6 pose blocks, lambda from 1e-3, / 10 (floor 1e-9) on an accepted step (the total
 * cost fell and every Pz stayed positive), x 10 on a rejected one; a reduced 9 x 9 system without
 * a Cholesky factor is a rejected iteration.  The pose step is the field pose's (w left-multiplied,
 * t' = t + dt), the intrinsics step additive; a value that is not free comes back bit for bit.
 * Start: cfg.init as given (guess = 0), or (guess = 1) fx, fy from the stored tags' homographies by
 * Zhang's two constraints per plane with the principal point at (width / 2, height / 2) and
 * distortion 0.  Each view starts from the stored tag whose homography pose under the start
 * intrinsics has the least reprojection error over the view's corners; a view where every
 * candidate has a corner behind the camera is skipped.
 *
 * at_camcal_create: AT_E_INVALID for a NULL, a free_mask outside 0..511, width, height or tag_size
 * not positive, guess = 0 with init.fx or init.fy not positive, a board at_set_field_layout would
 * refuse (or an empty one), max_hamming < 0.
 * at_camcal_add: one frame's detections; the field pose's selection over the board's ids is stored
 * (at most AT_FIELD_MAX_TAGS tags: id, corners, homography).  Returns 1 if a tag was stored, 0 if
 * none, AT_E_CAPACITY beyond AT_CAMCAL_MAX_VIEWS.
 * at_camcal_solve: the solve on the GPU (kernels k_cc_*, on a stream of the calibrator's own; one
 * synchronisation, at the end).  at_camcal_solve_host: the same on the CPU, the kernels'
 * arithmetic in the kernels' order: bit-equal records.  Both AT_E_INVALID without a stored view
 * or when the focal guess has no positive solution (e.g. every view fronto-parallel).
 * cov is sigma^2 times the inverse of the undamped reduced matrix at the final state, row-major
 * 9 x 9 in the mask's order, sigma^2 = cost / (2 corners - 6 views_used - free parameters); rows and
 * columns of parameters that are not free are zero; cov_valid = 0 (and zeros) without a factor or
 * with a denominator that is not positive.
 * at_camcal_views: per stored view of the last solve, the board's final pose and RMS (used = 0:
 * skipped, rest zero); returns the count, writes at most cap.
 * at_camcal_stats, the last solve: [0] views used, [1] skipped, [2] accepted steps, [3] rejected
 * steps, [4] the kernels' time in nanoseconds (HIP events around the sequence of the last
 * at_camcal_solve while at_camcal_set_profiling is on, 0 otherwise). */
#define AT_CAMCAL_MAX_VIEWS 4096
#define AT_CAMCAL_FX 1
#define AT_CAMCAL_FY 2
#define AT_CAMCAL_CX 4
#define AT_CAMCAL_CY 8
#define AT_CAMCAL_K1 16
#define AT_CAMCAL_K2 32
#define AT_CAMCAL_P1 64
#define AT_CAMCAL_P2 128
#define AT_CAMCAL_K3 256
typedef struct {
  int32_t width, height;
  at_camera init;
  int32_t free_mask;
  int32_t guess;
} at_camcal_config;
typedef struct {
  at_camera cam;
  double cov[81];
  double rms_before, rms_after;        /* pixels, over the corners of the views used */
  int32_t views_used, views_skipped;
  int32_t corners;
  int32_t accepted, rejected;
  int32_t cov_valid;
} at_camcal_result;
typedef struct {
  double R[9]; double t[3];            /* x_cam = R x_board + t */
  double rms_px;
  int32_t n_tags, used;
} at_camcal_view;
typedef struct at_camcal at_camcal;
int at_camcal_create(const at_camcal_config *cfg, const at_field_tag *board, int n_tags, int max_hamming,
                     double tag_size, at_camcal **out);
int at_camcal_add(at_camcal *c, const at_detection *dets, int n);
int at_camcal_count(const at_camcal *c);
int at_camcal_clear(at_camcal *c);
int at_camcal_solve(at_camcal *c, at_camcal_result *out);
int at_camcal_solve_host(at_camcal *c, at_camcal_result *out);
int at_camcal_views(const at_camcal *c, at_camcal_view *out, int cap);
int at_camcal_set_profiling(at_camcal *c, int on);
int at_camcal_stats(const at_camcal *c, uint64_t *out, int cap);
void at_camcal_destroy(at_camcal *c);

/* Field map: where the tags of a field really stand, from recorded views (bundle adjustment).
 *
 * A map is 1..AT_FIELDMAP_MAX_TAGS tags.  Each carries an at_field_tag (x_field = R x_tag + t), a
 * flag `known` (1: the given pose is its start, 0: there is none and R, t are not read) and the
 * flags free_rot / free_trans of what is to be solved for.  At least one tag must be known with
 * both flags 0: the anchor, which fixes where the field frame is.
 * Unknowns: the camera pose of every stored view that takes part (x_cam = R x_field + t) and the
 * free parts of every placed tag.  Cost: the summed squared error in pixels of every stored corner
 * of every placed tag against at_detection.p through the view's own fx, fy, cx, cy (p as k_pose
 * reads it: no further undistortion); a corner at Pz <= 0 costs infinity.  Parameters: per view
 * (w, dt) as the field pose (w left-multiplied, t' = t + dt); per tag (w_j, d_j) with
 * R_j' = R_j dR(w_j), t_j' = t_j + d_j.  16 Levenberg-Marquardt iterations on the whole problem
 * through the Schur complement of the views' 6 x 6 pose blocks, the reduced system (6 per tag)
 * assembled sparsely, block pair by block pair; lambda from 1e-3, / 10 (floor 1e-9) on an accepted
 * step (the total cost fell and every Pz stayed positive), x 10 on a rejected one; a reduced
 * system without a Cholesky factor is a rejected iteration.  A part that is not free comes back
 * bit for bit.
 * Placing: a tag with known = 0 gets its start from views that see it together with tags already
 * placed, in rounds over ascending ids until nothing changes: per such view the camera pose by
 * the field pose's start rule over the view's placed tags, the candidate (cam_T_field)^-1
 * cam_T_tag, and of all candidates the one with the least summed squared reprojection error of the
 * tag's corners over all such views (ties: the lower view).  A tag no chain of views reaches is
 * not placed: placed = 0 and zeros in its record, and its observations take no part.
 * Every view starts from the field pose's solve over the placed tags' start poses; one that gets
 * none is skipped.  A component of the map without a fixed tag is not refused: it floats where
 * its start put it and its variances mean nothing (at_fieldmap.h).
 *
 * at_fieldmap_create: AT_E_INVALID for a NULL, n outside 1..AT_FIELDMAP_MAX_TAGS, an id outside
 * [0, 1024) or twice, no anchor, a known tag at_set_field_layout would refuse, max_hamming < 0,
 * tag_size not positive.
 * at_fieldmap_add: one frame's at_detections / at_poses arrays and that frame's camera (fx, fy,
 * cx, cy are kept); the field pose's selection over the map's ids is stored (at most
 * AT_FIELD_MAX_TAGS tags, the lowest ids: id, corners, the tag's own pose).  Returns 1 if stored,
 * 0 if fewer than two map tags were selected (such a view constrains nothing), AT_E_CAPACITY
 * beyond AT_FIELDMAP_MAX_VIEWS.
 * at_fieldmap_solve: the solve on the GPU (kernels k_fm_*, on a stream of the mapper's own; one
 * synchronisation, at the end; it is in no detector's launch sequence and writes nothing of a
 * detector's).  at_fieldmap_solve_host: the same on the CPU, the kernels' arithmetic in the
 * kernels' order: bit-equal records.  Both AT_E_INVALID without a stored view.
 * cov of a tag is sigma^2 times its 6 x 6 diagonal block of the inverse of the undamped reduced
 * matrix at the final state, order (w_j, d_j) -- w_j a small turn in the tag frame, d_j in the
 * field frame -- sigma^2 = cost / (2 corners - 6 views_used - free parameters); rows and columns
 * of parameters that are not free are zero; cov_valid = 0 (and zeros) without a factor or with a
 * denominator that is not positive.
 * at_fieldmap_tags: per tag of the map, in the order given, of the last solve; at_fieldmap_views:
 * per stored view, its final camera pose and RMS (used = 0: skipped, rest zero).  Both return the
 * count and write at most cap.
 * at_fieldmap_stats, the last solve: [0] views used, [1] skipped, [2] accepted steps, [3] rejected
 * steps, [4] the kernels' time in nanoseconds (HIP events around the sequence of the last
 * at_fieldmap_solve while at_fieldmap_set_profiling is on, 0 otherwise), [5] candidates dropped by
 * the 16-tag cap over the stored views. */
#define AT_FIELDMAP_MAX_TAGS 32
#define AT_FIELDMAP_MAX_VIEWS 4096
typedef struct {
  at_field_tag tag;
  int32_t known;
  int32_t free_rot, free_trans;
  int32_t pad;
} at_fieldmap_tag;
typedef struct {
  int32_t id, placed;
  double R[9]; double t[3];            /* x_field = R x_tag + t, final */
  double R0[9]; double t0[3];          /* the start: where the caller or the chain put it */
  double cov[36];
  int32_t views, pad;                  /* stored views that hold the tag */
} at_fieldmap_tag_result;
typedef struct {
  double rms_before, rms_after;        /* pixels, over the corners of the views used */
  int32_t views_used, views_skipped;
  int32_t corners;
  int32_t accepted, rejected;
  int32_t cov_valid;
  int32_t n_tags, n_placed;
} at_fieldmap_result;
typedef struct {
  double R[9]; double t[3];            /* x_cam = R x_field + t */
  double rms_px;
  int32_t n_tags, used;
} at_fieldmap_view;
typedef struct at_fieldmap at_fieldmap;
int at_fieldmap_create(const at_fieldmap_tag *tags, int n, int max_hamming, double tag_size, at_fieldmap **out);
int at_fieldmap_add(at_fieldmap *m, const at_detection *dets, const at_pose *poses, int n, const at_camera *cam);
int at_fieldmap_count(const at_fieldmap *m);
int at_fieldmap_clear(at_fieldmap *m);
int at_fieldmap_solve(at_fieldmap *m, at_fieldmap_result *out);
int at_fieldmap_solve_host(at_fieldmap *m, at_fieldmap_result *out);
int at_fieldmap_tags(const at_fieldmap *m, at_fieldmap_tag_result *out, int cap);
int at_fieldmap_views(const at_fieldmap *m, at_fieldmap_view *out, int cap);
int at_fieldmap_set_profiling(at_fieldmap *m, int on);
int at_fieldmap_stats(const at_fieldmap *m, uint64_t *out, int cap);
void at_fieldmap_destroy(at_fieldmap *m);

/* Page-locked host memory (hipHostMalloc) for buffers the detector copies into on
 * its stream by DMA, e.g. at_annotate_staged's bgr_out: a pageable destination
 * goes through the runtime's staging buffers instead.  (No counterpart in the
 * reference: its node copies the image with cv_bridge, apriltags_cuda_detector.cu:514-518.)
 * Returns AT_OK / AT_E_NOMEM; at_host_free(NULL) is a no-op. */
int at_host_alloc(size_t bytes, void **out);
void at_host_free(void *p);

void at_destroy(at_detector *d);
const char *at_strerror(int code);

/* Family data (host only, no device needed). */
int at_family_num_known(const char *family);
int at_family_entry(const char *family, int i, int *id, uint64_t *code);

/* Library self-description. */
int at_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* AT_API_H_ */
