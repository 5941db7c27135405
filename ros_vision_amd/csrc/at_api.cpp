// at_api.cpp -- host side of the C ABI (include/at_api.h).
//
// Owns the device buffers (sized once, for max_batch frames at worst case,
// like GpuDetector's constructor, apriltag_gpu.cu:111-188), launches the
// kernel pipeline on one HIP stream and runs the small host tail: order the
// per-frame candidates by blob rank (the reference decodes quads in blob-index
// order, apriltag_detect.cu:642-658), reconcile_detections and zarray_sort by
// id (apriltag_detect.cu:660-662).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/at_api.h"
#include "at_common.h"
#include "at_gp.h"
#include "at_mjpg.h"
#include "at_mjpg_entropy.h"
#include "at_preview.h"
#include "at_rigcal.h"
#include "at_fieldmap.h"
#include "at_camcal.h"
#include "at_rigtrack.h"

namespace at {
hipError_t launch_tap_sizes(const uint8_t* thr, const uint32_t* par, const uint32_t* size, uint32_t* out, int Wd,
                            int Hd, hipStream_t st);
hipError_t launch_tap_labels(const uint8_t* thr, const uint32_t* par, uint32_t* out, int Wd, int Hd, hipStream_t st);
hipError_t launch_gp_preprocess(const uint8_t* src, int w, int h, float* out, int ow, int oh, int c, hipStream_t st);
hipError_t launch_draw(const DrawPrim* prims, int n, uint32_t* last, uint8_t* bgr, int W, int H, hipStream_t st);
hipError_t launch_preview(const uint8_t* src, int fmt, int W, int H, int s, uint8_t* dst, hipStream_t st);
hipError_t launch_mjpg_idct(const uint8_t* coef, size_t slot, uint8_t* out, size_t out_stride, int W, int H,
                            int nframes, hipStream_t st);
hipError_t launch_mjpg_color(const uint8_t* coef, size_t slot, const uint8_t* gray, uint8_t* planes,
                             size_t plane_stride, uint8_t* bgr, size_t img_stride, int W, int H, int nframes,
                             hipStream_t st);
hipError_t launch_mjpg_entropy(const EntBufs& b, int nframes, hipStream_t st);
hipError_t launch_jpg_encode(const uint8_t* bgr, int W, int H, int quality, int sampling, const JpgBufs& b,
                             hipStream_t st);
hipError_t launch_gp_parse(const float* raw, size_t frame_stride, int nframes, int P, int C, float conf_thr,
                           float iou_thr, float sx, float sy, const GpParseBufs& b, hipStream_t st);
hipError_t prepare_kernels(const Geom& g);
hipError_t launch_pipeline(const DevBufs& b, const Geom& g, const Params& prm, int B, int fmt, int nblobwg,
                           hipStream_t st, hipEvent_t* ev, hipStream_t st2, hipEvent_t fork, hipEvent_t join,
                           const KernelTimer* kt, const FieldLaunch* field);
// (at_fieldpose.cpp)
int fp_build_layout(const at_field_tag* tags, int n, int16_t* lut, std::vector<FpTag>* out);
void fp_write(const FpRecord& r, at_field_pose* o);
// (at_rigpose.cpp)
bool rig_extrinsics_ok(const at_rig_extrinsics& e);
void rig_write(const RigRecord& r, at_rig_pose* o);
bool rig_robust_config(const at_rig_robust_config* c, RigRobustCfg* out);
// (at_kernels.hip)
hipError_t launch_rig(const RigBufs& rb, int ninstants, hipStream_t st);
hipError_t launch_rig_robust(const RigBufs& rb, const RigRobustBufs& xb, int ninstants, hipStream_t st);
hipError_t launch_und_points(const UndCam& cam, const double* xy, int n, double* out, uint8_t* ok, hipStream_t st);
hipError_t launch_rigcal(const CalBufs& b, hipStream_t st);
hipError_t launch_camcal(const CcBufs& b, hipStream_t st);
hipError_t launch_fieldmap(const FmBufs& b, hipStream_t st);
hipError_t launch_rigtrack(const TrkBufs& b, const TrkTodo& todo, int iters, hipStream_t st, hipEvent_t* ev);

struct CodeEntry {
  int id;
  uint64_t code;
};
static const CodeEntry kTag36h11[] = {
#include "at_tag36h11_codes.inc"
};
static const CodeEntry kTag25h9[] = {
#include "at_tag25h9_codes.inc"
};
static const CodeEntry kTag16h5[] = {
#include "at_tag16h5_codes.inc"
};

// The families setup_tag_family selects by name (apriltag_utils.cu:10-32).  The
// classic square ones are built: d x d data cells, a one-cell black border
// (width_at_border d + 2), a white quiet zone (total_width d + 4), normal border,
// 2 bits corrected (apriltag_detector_add_family).  The apriltag 3 layouts
// (tagCircle21h7, tagCircle49h12, tagStandard41h12, tagStandard52h13,
// tagCustom48h12) are named but have no codebook here: their tables live in the
// un-vendored upstream sources and could not be regenerated offline, so
// at_create reports AT_E_FAMILY for them.
struct FamilyInfo {
  const char* name;
  int d;
  const CodeEntry* codes;
  int ncodes;
};
#define AT_NCODES(a) ((int)(sizeof(a) / sizeof((a)[0])))
static const FamilyInfo kFamilies[] = {
    {"tag36h11", 6, kTag36h11, AT_NCODES(kTag36h11)},
    {"tag25h9", 5, kTag25h9, AT_NCODES(kTag25h9)},
    {"tag16h5", 4, kTag16h5, AT_NCODES(kTag16h5)},
};

static const FamilyInfo* find_family(const char* name) {
  if (!name) return nullptr;
  for (const FamilyInfo& f : kFamilies)
    if (!strcmp(f.name, name)) return &f;
  return nullptr;
}

// apriltag_family_t fields quad_decode_index reads; bit_x / bit_y in the 3.x
// layout of tagXXhY.c: the upper triangle of the top-left quadrant row by row,
// rotated by 90 degrees three more times ((x, y) -> (d+1-y, x)), the centre
// cell last when d is odd
static FamilyDesc family_desc(const FamilyInfo& f) {
  FamilyDesc fd{};
  const int d = f.d;
  fd.nbits = d * d;
  fd.width_at_border = d + 2;
  fd.total_width = d + 4;
  fd.reversed_border = 0;
  fd.ncodes = f.ncodes;
  int n = 0;
  for (int r = 0; r < 4; r++)
    for (int y = 1; y <= d / 2; y++)
      for (int x = y; x <= d - y; x++) {
        int xx = x, yy = y;
        for (int i = 0; i < r; i++) {
          const int t = xx;
          xx = d + 1 - yy;
          yy = t;
        }
        fd.bitx[n] = (int8_t)xx;
        fd.bity[n] = (int8_t)yy;
        n++;
      }
  if (d & 1) {
    fd.bitx[n] = (int8_t)(d / 2 + 1);
    fd.bity[n] = (int8_t)(d / 2 + 1);
  }
  return fd;
}
}  // namespace at

using namespace at;

static_assert(kMjpgInvalid == AT_E_INVALID && kMjpgUnsupported == AT_E_UNSUPPORTED && kMjpgOk == AT_OK,
              "at_mjpg.h carries the ABI's codes");
static_assert(kFpMaxIds == kMaxCodes && kMaxDets <= kFpMaxCand, "at_fieldpose.h: ids and candidate slots of a frame");
static_assert(kJpg420 == AT_JPEG_420 && kJpg422 == AT_JPEG_422 && kJpg444 == AT_JPEG_444 && AT_E_CAPACITY == -3,
              "at_mjpg.h carries the ABI's sampling codes");

// control block layout (u32 words, zeroed every batch): per-frame arrays of B
// words, then scalars
enum { kCtlNpts, kCtlNpairs, kCtlNdets, kCtlNquads, kCtlStatus, kCtlNpent, kCtlNqcand, kCtlCclOvf, kCtlNlr,
       kCtlPerFrame };
enum { kCtlWorkhead = 0, kCtlQhead = 1, kCtlWorkheadSmall = 2, kCtlBlobPts = 3, kCtlNcls = 5,
       kCtlDetHead = kCtlNcls + kNumCls, kCtlDecDone = kCtlDetHead + 1, kCtlWorkheadMid = kCtlDecDone + 1,
       kCtlScalars = kCtlWorkheadMid + 1 };

static constexpr unsigned kTimingEventFlags = hipEventDisableSystemFence;

struct at_detector {
  at_config cfg;
  at_camera cam;
  Geom g;
  Params prm;
  int B;
  int device;
  int nblobwg;
  hipStream_t st;
  hipStream_t st2;          // fork/join branch for the large-blob kernel (latency mode)
  hipEvent_t ev_fork, ev_join;
  DevBufs d;
  std::vector<void*> allocs;
  uint8_t* d_in;            // staging for host frames [B][max frame bytes]
  size_t in_stride;
  const uint8_t** h_ftab;   // frame pointer table (mapped, fine-grained host memory; k_pre reads it)
  uint32_t* d_ctrl;         // control block (zeroed each batch)
  size_t ctrl_words;
  size_t kstamp_word;       // first of the timed kernel's stamp words in the control block
  double wclk_khz;          // device wall clock (s_memrealtime) rate
  double kd_ms;             // device-clock spans of the timed kernel (sum) and their count
  long long kd_n;
  uint32_t* h_ctrl;         // pinned copy of the control block
  DevDetection* h_dets;     // pinned [B][kDetPoolPerFrame]: mirror of each frame's first candidates (mapped)
  // results of the last collected batch: frame f's detections are the records
  // res_base[f][res_idx[f * kMaxDets + i]], i < res_n[f], in id order (after reconcile);
  // res_base[f] is the frame's host mirror, or res_ovf[f] (its candidates copied from
  // HBM) when it had more than kDetPoolPerFrame
  std::vector<int> res_idx, res_n;
  std::vector<const DevDetection*> res_base;
  std::vector<std::vector<DevDetection>> res_ovf;
  int last_nframes;
  int last_fmt;
  int last_gray;            // the last batch wrote the gray plane (AT_STAGE_GRAY)
  int last_sizes;           // ... and the size plane (AT_STAGE_SIZES)
  int last_staged;          // the last batch's frames were host frames staged in d_in (at_detect*)
  int last_gp;              // the last batch produced the game-piece tensors (k_gp_pre; a colour MJPG batch: k_gp_pre_one)
  int last_mj_color;        // the last batch was an MJPG batch enqueued with colour on (d_mj_bgr holds its images)
  int pending;
  hipEvent_t ev_done;
  hipEvent_t ev_ext;                      // at_stream_wait: recorded on the producer's stream
  int use_graphs;                         // replay the launch sequence as a hipGraph (AT_NO_GRAPH=1 disables)
  std::map<int, hipGraphExec_t> graphs;   // key: nframes * 4 + fmt
  // kernel timer under graph replay: the sequence cut around the timed kernel into
  // three graphs, timing events recorded between them (key: graph key * 32 + stage)
  struct SplitGraphs { hipGraphExec_t seg[3]; };
  std::map<int, SplitGraphs> split_graphs;
  std::vector<hipGraph_t> cap_segs;      // segments collected during one capture
  KernelTimer kt;                         // kt.stage < 0: off
  double kt_ms;
  long long kt_n;
  int profiling;
  hipEvent_t ev_stage[kNumStages + 1];
  double stage_ms[kNumStages];
  long stage_batches;
  double host_wait_us, host_tail_us;  // cumulative time of at_collect in the event wait / the host tail
  // annotated image (at_draw_outlines_device): segments, last-writer plane (lazily allocated)
  DrawPrim* d_prims;
  size_t prims_cap;
  uint32_t* d_last;
  // MJPG input (at_enqueue_mjpg), allocated on the first MJPG call for max_batch frames:
  // coefficient streams [B][mj_slot] in HBM and two page-locked staging sets of the same
  // shape, used in turn -- the host decodes a batch into one set while the copy of the
  // batch before may still be reading the other
  uint8_t* mj_host[2];
  uint8_t* d_mj;
  size_t mj_slot;
  int mj_cur;               // staging set of the last enqueued MJPG batch
  int mj_threads;           // host decode threads per batch (at_mjpg_set_threads)
  std::vector<at::MjpgDecoder> mj_dec;  // one decoder (with its scratch lists) per thread
  std::vector<int> mj_rc;
  std::vector<size_t> mj_bytes;   // per frame: bytes of its coefficient stream
  std::vector<uint8_t> mj_dense;  // ... and whether it took the dense encoding
  uint64_t mj_stats[9];     // last MJPG batch: compressed bytes, bytes sent, dense frames, decode us, kernel ns,
                            // colour kernels ns, entropy kernel ns, host-route frames, most sync rounds
  hipEvent_t ev_mj[3];      // around k_mjpg_idct, and after the colour kernels, while stage profiling is on
                            // (created on first use)
  int mj_timed;             // the pending batch recorded them (2: the colour one too)
  // colour (at_mjpg_set_color), allocated on the first colour-on MJPG call, when the slots above
  // grow to hold the chroma sub-streams: two chroma planes per frame and the BGR8 images
  int mj_color;             // the setting; takes effect at the next at_enqueue_mjpg
  int mj_color_bufs;        // the buffers are the colour-sized ones
  uint8_t* d_mj_planes;     // [B][2][mj_plane]
  size_t mj_plane;
  uint8_t* d_mj_bgr;        // [B][in_stride]
  // entropy decode on the device (at_mjpg_set_device_entropy), allocated on the first MJPG call
  // with the switch on: the batch as it crosses the link (a directory, then per frame its record
  // and scan bytes; two page-locked staging sets used in turn like mj_host) and k_mjpg_entropy's
  // scratch
  int mj_dev_ent;           // the setting; takes effect at the next at_enqueue_mjpg
  int mj_subseq;            // piece size S in bytes
  uint8_t* mj_ent_host[2];
  size_t mj_ent_cap;        // bytes of one set, and of the device copy
  at::EntBufs ent;          // (ent.in: the device copy)
  uint32_t* h_ent_info;     // page-locked copy of ent.info
  int mj_ent_batch;         // the pending / last batch went through k_mjpg_entropy (h_ent_info is its status)
  hipEvent_t ev_ent[2];     // around k_mjpg_entropy while stage profiling is on (created on first use)
  int mj_ent_timed;
  // JPEG output (at_encode_jpeg_device), allocated on the first call at the worst case of
  // this geometry (4:4:4, every block at its longest, every byte stuffed) and kept
  at::JpgBufs jpg;
  size_t jpg_out_cap;       // bytes of jpg.out
  uint32_t* h_jpg_total;    // mapped, page-locked: where k_jpg_pack leaves the length
  uint8_t jpg_hdr[at::kJpgHeaderMax];  // SOI .. SOS of the last (quality, sampling, width, height)
  size_t jpg_hdr_len;
  int jpg_hdr_q, jpg_hdr_s, jpg_hdr_w, jpg_hdr_h;
  uint64_t jpg_stats[2];    // last encode: bytes out, the encode kernels' ns (while profiling)
  hipEvent_t ev_jpg[2];     // around them (created on first use)
  // game-piece output parse (at_gp_parse_device), allocated on the first call for max_batch
  // frames and kept: candidate lists in HBM, boxes and counts in mapped page-locked memory
  at::GpParseBufs gp;
  at::GpBox* h_gp_out;      // [B][kGpMaxCand] the host side of gp.out
  uint32_t* h_gp_info;      // [B][2] ... and of gp.info: boxes kept, candidates
  uint64_t gp_stats[4];     // last call: candidates, most of one frame, boxes kept, kernel ns (while profiling)
  hipEvent_t ev_gp[2];      // around the two kernels (created on first use)
  // preview (at_preview_bgr / at_preview_jpeg): the pw x ph BGR8 image, allocated on the first
  // call at width * height * 3 (s = 1) and kept
  uint8_t* d_pv;
  uint64_t pv_stats[6];     // last call: bytes, quality used, encodes, pw, ph, kernels' ns (while profiling)
  hipEvent_t ev_pv[2];      // around k_preview and the drawing (created on first use)
  // field pose (at_set_field_layout): the layout in HBM (id table, tags; allocated on the first
  // call at kMaxCodes entries and kept), one record per frame in HBM and in mapped host memory
  FieldLaunch field;        // field.b: what k_field gets; field.ev: around it while stage profiling is on
  int field_on;             // a layout is set: later batches run k_field
  int last_field;           // the pending / last batch ran it (h_field holds its records)
  int field_timed;          // ... and recorded ev_field
  FpRecord* h_field;        // [B] the host side of field.b.hout
  hipEvent_t ev_field[2];   // (created on first use)
  uint64_t field_ns;        // k_field's time of the last collected batch (while profiling)
  // ideal corners (at_set_undistort): d.und / d.hund, allocated on the first call and kept
  int last_und;             // the pending / last batch ran with the mode on (h_und holds its records)
  UndRecord* h_und;         // [B][kDetPoolPerFrame] the host side of d.hund
  std::vector<std::vector<UndRecord>> und_ovf;  // a frame of more than kDetPoolPerFrame candidates: copied from HBM on demand
  void* d_undpts;           // at_undistort_points' staging (in, out, flags), grown on demand
  size_t undpts_cap;        // points it holds
};

// Experiment and diagnostic knobs (stage cut-offs, grid / tile overrides, phase
// probes, graph / fork switches) are read from the environment only by a build
// with -DAT_EXPERIMENTS (`make exp`, the A/B tools' library): a product build
// ignores the environment, so no variable can truncate the pipeline of a deployed
// detector (the reference either detects or aborts, cuda_frc971.h:14-17).
static const char* knob(const char* name) {
#ifdef AT_EXPERIMENTS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
static int knob_int(const char* name, int dflt) {
  const char* v = knob(name);
  return v ? atoi(v) : dflt;
}

static int hip_fail(hipError_t e) {
  if (e != hipSuccess) {
    fprintf(stderr, "at_api: HIP error %s\n", hipGetErrorString(e));
    return AT_E_HIP;
  }
  return AT_OK;
}
#define HIPCHK(x)                          \
  do {                                     \
    hipError_t e_ = (x);                   \
    if (e_ != hipSuccess) return hip_fail(e_); \
  } while (0)

extern "C" {

int at_abi_version(void) { return AT_ABI_VERSION; }

const char* at_strerror(int code) {
  switch (code) {
    case AT_OK: return "ok";
    case AT_E_INVALID: return "invalid argument or unsupported frame geometry";
    case AT_E_HIP: return "HIP runtime error";
    case AT_E_CAPACITY: return "frame exceeded a fixed capacity";
    case AT_E_FAMILY: return "unknown tag family";
    case AT_E_NOMEM: return "out of memory";
    case AT_E_UNSUPPORTED: return "unsupported JPEG stream (not baseline 8-bit 4:4:4 / 4:2:2 / 4:2:0 / gray)";
    default: return "unknown error";
  }
}

int at_family_num_known(const char* family) {
  const FamilyInfo* f = find_family(family);
  return f ? f->ncodes : AT_E_FAMILY;
}

int at_family_entry(const char* family, int i, int* id, uint64_t* code) {
  const FamilyInfo* f = find_family(family);
  if (!f) return AT_E_FAMILY;
  if (i < 0 || i >= f->ncodes) return AT_E_INVALID;
  if (id) *id = f->codes[i].id;
  if (code) *code = f->codes[i].code;
  return AT_OK;
}

int at_config_default(at_config* cfg, int width, int height) {
  if (!cfg) return AT_E_INVALID;
  memset(cfg, 0, sizeof(*cfg));
  cfg->width = width;
  cfg->height = height;
  cfg->family = "tag36h11";
  cfg->quad_decimate = 2.0f;
  cfg->refine_edges = 1;
  cfg->decode_sharpening = 0.25;
  cfg->min_white_black_diff = 5;
  cfg->min_cluster_pixels = 5;
  cfg->max_nmaxima = 10;
  cfg->max_line_fit_mse = 10.0f;
  cfg->cos_critical_rad = cos(10.0 * M_PI / 180.0);
  cfg->device = 0;
  cfg->max_batch = 1;
  cfg->tag_size = 0.1651;  // TAGSIZE, apriltags_cuda_detector.hpp:39
  return AT_OK;
}

void at_destroy(at_detector* d) {
  if (!d) return;
  (void)hipSetDevice(d->device);
  if (d->st) (void)hipStreamSynchronize(d->st);
  if (d->st2) (void)hipStreamSynchronize(d->st2);
  for (auto& kv : d->graphs) (void)hipGraphExecDestroy(kv.second);
  d->graphs.clear();
  for (auto& kv : d->split_graphs)
    for (auto* g : kv.second.seg) (void)hipGraphExecDestroy(g);
  d->split_graphs.clear();
  for (void* p : d->allocs) (void)hipFree(p);
  if (d->h_ftab) (void)hipHostFree(d->h_ftab);
  if (d->h_ctrl) (void)hipHostFree(d->h_ctrl);
  if (d->h_dets) (void)hipHostFree(d->h_dets);
  if (d->d_prims) (void)hipFree(d->d_prims);
  if (d->d_last) (void)hipFree(d->d_last);
  for (uint8_t* p : d->mj_host)
    if (p) (void)hipHostFree(p);
  for (hipEvent_t e : d->ev_mj)
    if (e) (void)hipEventDestroy(e);
  for (uint8_t* p : d->mj_ent_host)
    if (p) (void)hipHostFree(p);
  if (d->h_ent_info) (void)hipHostFree(d->h_ent_info);
  for (hipEvent_t e : d->ev_ent)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : d->ev_jpg)
    if (e) (void)hipEventDestroy(e);
  if (d->h_jpg_total) (void)hipHostFree(d->h_jpg_total);
  for (hipEvent_t e : d->ev_gp)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : d->ev_pv)
    if (e) (void)hipEventDestroy(e);
  if (d->d_pv) (void)hipFree(d->d_pv);
  for (hipEvent_t e : d->ev_field)
    if (e) (void)hipEventDestroy(e);
  if (d->h_field) (void)hipHostFree(d->h_field);
  if (d->h_und) (void)hipHostFree(d->h_und);
  if (d->d_undpts) (void)hipFree(d->d_undpts);
  if (d->h_gp_out) (void)hipHostFree(d->h_gp_out);
  if (d->h_gp_info) (void)hipHostFree(d->h_gp_info);
  if (d->ev_done) (void)hipEventDestroy(d->ev_done);
  if (d->ev_ext) (void)hipEventDestroy(d->ev_ext);
  for (int i = 0; i <= kNumStages; i++)
    if (d->ev_stage[i]) (void)hipEventDestroy(d->ev_stage[i]);
  if (d->kt.t0) (void)hipEventDestroy(d->kt.t0);
  if (d->kt.t1) (void)hipEventDestroy(d->kt.t1);
  if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
  if (d->ev_join) (void)hipEventDestroy(d->ev_join);
  if (d->st2) (void)hipStreamDestroy(d->st2);
  if (d->st) (void)hipStreamDestroy(d->st);
  delete d;
}

int at_create(const at_config* cfg, const at_camera* cam, at_detector** out) {
  if (!cfg || !cam || !out) return AT_E_INVALID;
  *out = nullptr;
  const FamilyInfo* fam = find_family(cfg->family);
  if (!fam || fam->ncodes > kMaxCodes) return AT_E_FAMILY;
  const int W = cfg->width, H = cfg->height;
  // GpuDetector preconditions (apriltag_gpu.cu:166-167, 754-755, 774; line_fit_filter.cu:1205)
  if (W <= 16 || H <= 16 || W % 8 || H % 8 || (long)W * H >= (1L << 22)) return AT_E_INVALID;
  if (cfg->quad_decimate != 2.0f || cfg->max_nmaxima != 10 || cfg->max_batch < 1 || cfg->max_batch > kMaxBatch)
    return AT_E_INVALID;
  if (2 * (W + H) > kSortCap) return AT_E_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device) return AT_E_HIP;
  at_detector* d = new at_detector();  // value-initialised: every pointer null
  d->cfg = *cfg;
  d->cfg.family = fam->name;
  d->cam = *cam;
  d->device = cfg->device;
  d->B = cfg->max_batch;
  d->mj_threads = 1;
  d->mj_subseq = at::kEntSubseqDefault;
  Geom& g = d->g;
  g.W = W; g.H = H; g.Wd = W / 2; g.Hd = H / 2;
  g.TW = g.Wd / 4; g.TH = g.Hd / 4;
  g.BW = g.Wd / 2; g.BH = g.Hd / 2;
  g.ctw = d->B < kWideBlobMaxBatch ? 32 : 64;
  if (knob("AT_CCL_TILE")) g.ctw = knob_int("AT_CCL_TILE", 64) == 32 ? 32 : 64;
  // size classes of the workgroup-team blob kernel (the rest: one wave per blob);
  // latency mode gives the team blobs of more than 256 points too (its chain is
  // the slowest single blob)
  g.nlarge = g.ctw == 32 ? std::max(kNumLargeCls, std::min(kNumCls, knob_int("AT_NLARGE", kNumLargeCls)))
                        : kNumLargeCls;  // (experiment knob: 3..kNumCls)
  g.CTX = (g.Wd + g.ctw - 1) / g.ctw;
  g.CTY = (g.Hd + kCclTileH - 1) / kCclTileH;
  // throughput mode: the cross-tile merge of the CCL in one workgroup's LDS per
  // frame (k_ccl_merge), room for 80 listed local roots per tile (typical 720p
  // frames list ~40), at most what 160 KiB hold; latency mode keeps the
  // multi-workgroup border / roots kernels (one frame: their parallelism is the chain)
  g.merge_cap = g.ctw == 64 ? std::min(kMergeCapMax, 80 * g.CTX * g.CTY) : 0;
  // 12 B per root (parent key + pixel count) and the wave link lists (8 KB)
  g.merge_lds = std::min(g.merge_cap * 12 + 8192, kMergeLdsMax);
  if (g.CTX * g.CTY > kMaxCclTiles) {
    at_destroy(d);
    return AT_E_INVALID;
  }
  g.cap_pts = 4 * (g.Wd - 2) * (g.Hd - 2);
  g.BTX = (g.Wd - 2 + 63) / 64;
  g.BTY = (g.Hd - 2 + 4 * kBndRows - 1) / (4 * kBndRows);
  g.ntb = g.BTX * g.BTY;
  g.bnd_region = kBndPts;
  g.bnd_region = std::max(kBndStage, std::min(kBndPts, knob_int("AT_BND_REGION", kBndPts)));  // (experiment knob)
  if (g.ntb > kMaxTilesPerFrame) {
    at_destroy(d);
    return AT_E_INVALID;
  }
  g.min_cluster = (uint32_t)std::max(24, cfg->min_cluster_pixels);
  g.max_cluster = (uint32_t)(2 * (W + H));
  // GpuDetector ctor (apriltag_gpu.cu:169-181): width_at_border / quad_decimate, >= 3
  g.min_tag_width = std::max(3, (fam->d + 2) / 2);
  Params& p = d->prm;
  p.min_white_black_diff = cfg->min_white_black_diff;
  p.max_line_fit_mse = cfg->max_line_fit_mse;
  p.cos_critical_rad = cfg->cos_critical_rad;
  p.decode_sharpening = cfg->decode_sharpening;
  p.refine_edges = cfg->refine_edges;
  p.fx = cam->fx; p.fy = cam->fy; p.cx = cam->cx; p.cy = cam->cy;
  p.k1 = cam->k1; p.k2 = cam->k2; p.p1 = cam->p1; p.p2 = cam->p2; p.k3 = cam->k3;
  p.diag_stop = knob_int("AT_DIAG_BLOB_STOP", 0);
  p.probe = knob_int("AT_PHASE_PROBE", 0);
  p.taps = 0;  // debug taps off: at_set_debug_taps
  p.wide_blob = knob_int("AT_WIDE_BLOB", 0);
  p.pipe_stop = knob_int("AT_DIAG_PIPE_STOP", 0);
  p.lblob_wg = knob("AT_LBLOB_WG") ? std::max(16, knob_int("AT_LBLOB_WG", 0)) : 0;  // experiment
  p.sblob_wg = knob("AT_SBLOB_WG") ? std::max(16, knob_int("AT_SBLOB_WG", 0)) : 0;  // experiment
  p.dec_wg = knob("AT_DEC_WG") ? std::max(16, knob_int("AT_DEC_WG", 0)) : 0;  // experiment
  p.dec_lpq = knob_int("AT_DEC_LPQ", 0) == 64 ? 64 : 0;  // experiment (16 is the product's)
  p.fam = family_desc(*fam);
  d->use_graphs = !knob_int("AT_NO_GRAPH", 0);
  if (!(cfg->tag_size >= 0) || !std::isfinite(cfg->tag_size)) {
    at_destroy(d);
    return AT_E_INVALID;
  }
  p.tag_size = cfg->tag_size;

  auto fail = [&](int code) {
    at_destroy(d);
    return code;
  };
  if (hipSetDevice(d->device) != hipSuccess) return fail(AT_E_HIP);
  if (hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking) != hipSuccess) return fail(AT_E_HIP);
  if (hipEventCreateWithFlags(&d->ev_done, hipEventDisableTiming) != hipSuccess) return fail(AT_E_HIP);
  if (hipEventCreateWithFlags(&d->ev_ext, hipEventDisableTiming) != hipSuccess) return fail(AT_E_HIP);
  // Latency mode (max_batch < kWideBlobMaxBatch): the small-blob kernel runs on a
  // second stream beside the large-blob one.  Throughput mode: both on the one
  // stream -- concurrency comes from several detector instances (batches in
  // flight), which then each need one hardware queue only.  AT_NO_FORK=1 forces
  // the single-stream form.
  const bool fork = d->B < kWideBlobMaxBatch && !knob_int("AT_NO_FORK", 0);
  if (fork && hipStreamCreateWithFlags(&d->st2, hipStreamNonBlocking) != hipSuccess) return fail(AT_E_HIP);
  if (hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming) != hipSuccess) return fail(AT_E_HIP);
  if (hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming) != hipSuccess) return fail(AT_E_HIP);
  d->kt.stage = -1;
  d->kt.split = nullptr;
  d->kt.ctx = nullptr;
  // timing-only events: no system-scope fence (cache writeback) when they complete,
  // so bracketing a kernel does not slow it or its neighbours on other streams
  if (hipEventCreateWithFlags(&d->kt.t0, kTimingEventFlags) != hipSuccess ||
      hipEventCreateWithFlags(&d->kt.t1, kTimingEventFlags) != hipSuccess)
    return fail(AT_E_HIP);
  int ncu = 0;
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, d->device);
  int wclk = 0;
  (void)hipDeviceGetAttribute(&wclk, hipDeviceAttributeWallClockRate, d->device);
  d->wclk_khz = wclk > 0 ? (double)wclk : 100000.0;  // s_memrealtime: 100 MHz
  d->nblobwg = std::max(64, ncu * 2);
  if (knob("AT_BLOB_WG")) d->nblobwg = std::max(16, knob_int("AT_BLOB_WG", 0));  // experiment: persistent grid size

  const size_t B = (size_t)d->B;
  const size_t npix = (size_t)W * H, nd = (size_t)g.Wd * g.Hd, nt = (size_t)g.TW * g.TH * 2;
  bool oom = false;
  auto dalloc = [&](size_t bytes) -> void* {
    void* ptr = nullptr;
    if (hipMalloc(&ptr, std::max<size_t>(bytes, 256)) != hipSuccess) {
      oom = true;
      return nullptr;
    }
    d->allocs.push_back(ptr);
    return ptr;
  };
  d->in_stride = (npix * 3 + 255) & ~(size_t)255;
  d->d_in = (uint8_t*)dalloc(B * d->in_stride);
  DevBufs& b = d->d;
  b.gray = (uint8_t*)dalloc(B * npix);
  b.dec = (uint8_t*)dalloc(B * nd);
  b.mm = (uint8_t*)dalloc(B * nt);
  b.thr = (uint8_t*)dalloc(B * nd);
  b.par = (uint32_t*)dalloc(B * nd * 4);
  b.lroot = (uint32_t*)dalloc(B * (size_t)g.CTX * g.CTY * kCclTileNodesMax * 4);
  b.nlroot = (uint32_t*)dalloc(B * (size_t)g.CTX * g.CTY * 4);
  b.lcnt = (uint32_t*)dalloc(B * (size_t)g.CTX * g.CTY * kCclTileNodesMax * 4);
  b.cdesc = (uint32_t*)dalloc(B * (size_t)g.CTX * g.CTY * CclDesc::kWords * 4);
  b.size = (uint32_t*)dalloc(B * nd * 4);
  const size_t ntb = (size_t)g.ntb;
  b.pts = (uint64_t*)dalloc(B * ntb * (size_t)g.bnd_region * 8);
  b.tcnt = (uint32_t*)dalloc(B * ntb * 4);
  b.tent = (uint32_t*)dalloc(B * ntb * 4);
  b.grp = (uint32_t*)dalloc(B * g.cap_pts * 4);
  b.keys = (uint64_t*)dalloc(B * g.cap_pts * 8);
  b.pent_key = (uint64_t*)dalloc(B * ntb * kLdsPairSlots * 8);
  b.pent_cnt = (uint32_t*)dalloc(B * ntb * kLdsPairSlots * 4);
  b.povf_key = (uint64_t*)dalloc(B * kPairEntCap * 8);
  b.povf_cnt = (uint32_t*)dalloc(B * kPairEntCap * 4);
  b.ht_key = (uint64_t*)dalloc(B * kHashSlots * 8);
  b.ht_cnt = (uint32_t*)dalloc(B * kHashSlots * 4);
  b.ht_rank = (uint32_t*)dalloc(B * kHashSlots * 4);
  b.ht_off = (uint32_t*)dalloc(B * kHashSlots * 4);
  b.ht_cur = (uint32_t*)dalloc(B * kHashSlots * 4);
  b.pair_cnt = (uint32_t*)dalloc(B * kMaxPairs * 4);
  b.pair_off = (uint32_t*)dalloc(B * kMaxPairs * 4);
  b.pair_sel = (uint32_t*)dalloc(B * kMaxPairs * 4);
  b.wcap = (uint32_t)(B * kMaxPairs);
  b.work = (uint32_t*)dalloc((size_t)kNumCls * B * kMaxPairs * 4);
  b.probe = (uint64_t*)dalloc(kProbeWords * 8);
  b.dets = (DevDetection*)dalloc(B * kMaxDets * sizeof(DevDetection));
  b.det_work = (uint32_t*)dalloc(B * kMaxDets * 4);
  b.quads = (QuadRecord*)dalloc(B * kMaxPairs * sizeof(QuadRecord));
  b.fpend = (FitPend*)dalloc(B * kMaxPairs * sizeof(FitPend));
  // control block: per-frame words, scalars, then (8-byte aligned) the timed
  // kernel's two wall-clock stamps and its finished-workgroup count
  d->kstamp_word = (kCtlPerFrame * B + kCtlScalars + 1) & ~(size_t)1;
  d->ctrl_words = d->kstamp_word + 5;
  d->d_ctrl = (uint32_t*)dalloc(((d->ctrl_words * 4 + 15) / 16) * 16);
  b.npts = d->d_ctrl + kCtlNpts * B;
  b.npairs = d->d_ctrl + kCtlNpairs * B;
  b.ndets = d->d_ctrl + kCtlNdets * B;
  b.nquads = d->d_ctrl + kCtlNquads * B;
  b.status = d->d_ctrl + kCtlStatus * B;
  b.npent = d->d_ctrl + kCtlNpent * B;
  b.qc_words = (uint32_t)(B * kQcStride);
  b.nqcand = (uint32_t*)dalloc((size_t)b.qc_words * 4);
  b.ccl_ovf = d->d_ctrl + kCtlCclOvf * B;
  b.nlr_tot = d->d_ctrl + kCtlNlr * B;
  uint32_t* sc = d->d_ctrl + kCtlPerFrame * B;
  b.workhead = sc + kCtlWorkhead;
  b.qhead = sc + kCtlQhead;
  b.workhead_small = sc + kCtlWorkheadSmall;
  b.workhead_mid = sc + kCtlWorkheadMid;
  b.blob_pts = sc + kCtlBlobPts;
  b.ncls = sc + kCtlNcls;
  b.det_head = sc + kCtlDetHead;
  b.dec_done = sc + kCtlDecDone;
  b.kt_stage = -1;
  b.kstamp = reinterpret_cast<uint64_t*>(d->d_ctrl + d->kstamp_word);
  b.kgrid = d->d_ctrl + d->kstamp_word + 4;
  b.kwg_cap = (uint32_t)(B * 1024 + 4096);  // >= the workgroups of any stamped launch (1080p: 510 tiles per frame)
  b.kwg = (uint64_t*)dalloc((size_t)b.kwg_cap * 2 * 8);
  b.qcand_cap = (uint32_t)(B * kQuadCandPerFrame);
  b.qcand = (QuadCand*)dalloc((size_t)b.qcand_cap * sizeof(QuadCand));
  // overflow area for the peak keys of pathological large blobs (one per large-blob team)
  b.s_pk = (uint64_t*)dalloc((size_t)2 * d->nblobwg * (kSortCap / 2) * 8);  // a slot per team (<= 2 nblobwg teams)
  // refine samples past LDS, one region per k_decode workgroup (throughput mode, where
  // launch_pipeline packs four quads into a wave: per row of a workgroup's wave) of the
  // grid launch_pipeline uses for a full batch (decode_grid; AT_DEC_WG can only lower it)
  b.rsamp = (double*)dalloc(decode_scratch_doubles(d->nblobwg, d->B, g.ctw == 64) * 8);
  if (oom) return fail(AT_E_NOMEM);
  if (prepare_kernels(g) != hipSuccess) return fail(AT_E_HIP);
  // frame pointer table: fine-grained mapped host memory read by k_pre directly
  // (no host-to-device copy per batch; the GPU does not cache it)
  if (hipHostMalloc((void**)&d->h_ftab, B * sizeof(void*), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
    return fail(AT_E_NOMEM);
  if (hipHostGetDevicePointer((void**)&b.frames, (void*)d->h_ftab, 0) != hipSuccess) return fail(AT_E_HIP);
  d->res_idx.assign(B * kMaxDets, 0);
  d->res_n.assign(B, 0);
  d->res_base.assign(B, nullptr);
  d->res_ovf.resize(B);
  if (hipHostMalloc((void**)&d->h_ctrl, d->ctrl_words * 4, hipHostMallocMapped) != hipSuccess) return fail(AT_E_NOMEM);
  if (hipHostMalloc((void**)&d->h_dets, B * kDetPoolPerFrame * sizeof(DevDetection), hipHostMallocMapped) != hipSuccess)
    return fail(AT_E_NOMEM);
  // device views of the mapped host result buffers (k_decode / k_pose write them)
  if (hipHostGetDevicePointer((void**)&b.hdets, d->h_dets, 0) != hipSuccess ||
      hipHostGetDevicePointer((void**)&b.hctrl, d->h_ctrl, 0) != hipSuccess)
    return fail(AT_E_HIP);
  b.ctrl = d->d_ctrl;
  b.ctrl_words = (uint32_t)d->ctrl_words;
  {
    // this detector's codebook in HBM (k_decode matches every entry in parallel)
    std::vector<uint64_t> codes(fam->ncodes);
    std::vector<int32_t> ids(fam->ncodes);
    for (int i = 0; i < fam->ncodes; i++) {
      codes[i] = fam->codes[i].code;
      ids[i] = fam->codes[i].id;
    }
    uint64_t* dc = (uint64_t*)dalloc(codes.size() * 8);
    int32_t* di = (int32_t*)dalloc(ids.size() * 4);
    if (oom) return fail(AT_E_NOMEM);
    if (hipMemcpy(dc, codes.data(), codes.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(di, ids.data(), ids.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return fail(AT_E_HIP);
    b.book_code = dc;
    b.book_id = di;
  }
  // size arrays are read for every label by k_boundary: start defined
  if (hipMemsetAsync(b.size, 0, B * nd * 4, d->st) != hipSuccess) return fail(AT_E_HIP);
  if (hipStreamSynchronize(d->st) != hipSuccess) return fail(AT_E_HIP);
  *out = d;
  return AT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// host tail: reconcile_detections + zarray_sort (apriltag 3.x apriltag.c,
// called at apriltag_detect.cu:660-662)
// ---------------------------------------------------------------------------
static bool seg_intersect(const double* a0, const double* a1, const double* b0, const double* b1) {
  const double ux = a1[0] - a0[0], uy = a1[1] - a0[1];
  const double vx = b1[0] - b0[0], vy = b1[1] - b0[1];
  const double den = ux * vy - uy * vx;
  if (fabs(den) < 1e-12) return false;
  const double t = ((b0[0] - a0[0]) * vy - (b0[1] - a0[1]) * vx) / den;
  const double w = ((b0[0] - a0[0]) * uy - (b0[1] - a0[1]) * ux) / den;
  return t >= 0 && t <= 1 && w >= 0 && w <= 1;
}
static bool poly_contains(const double poly[4][2], const double* pt) {
  bool inside = false;
  for (int i = 0, j = 3; i < 4; j = i++) {
    if (((poly[i][1] > pt[1]) != (poly[j][1] > pt[1])) &&
        (pt[0] < (poly[j][0] - poly[i][0]) * (pt[1] - poly[i][1]) / (poly[j][1] - poly[i][1]) + poly[i][0]))
      inside = !inside;
  }
  return inside;
}
static bool poly_overlap(const double a[4][2], const double b[4][2]) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      if (seg_intersect(a[i], a[(i + 1) & 3], b[j], b[(j + 1) & 3])) return true;
  return poly_contains(a, b[0]) || poly_contains(b, a[0]);
}
static int prefer_smaller(int pref, double q0, double q1) {
  if (pref) return pref;
  if (q0 < q1) return -1;
  if (q1 < q0) return 1;
  return 0;
}

static void write_detection(const DevDetection& v, at_detection* o) {
  o->id = v.id;
  o->hamming = v.hamming;
  o->decision_margin = v.decision_margin;
  memcpy(o->H, v.H, sizeof(o->H));
  memcpy(o->c, v.c, sizeof(o->c));
  memcpy(o->p, v.p, sizeof(o->p));
}

// One frame's candidates: idx[0..ncand) are pool indices; on return idx[0..n) are
// the detections in id order (n is returned).
static int host_tail(const DevDetection* cand, int* idx, int ncand, at_detection* out, int cap) {
  // the reference's zarray operations on an index array (the 280-byte records stay
  // where k_decode / k_pose wrote them): order by blob rank, reconcile with the
  // same swap-with-last removals, stable sort by id
  std::stable_sort(idx, idx + ncand, [&](int a, int b) { return cand[a].blob_rank < cand[b].blob_rank; });
  int n = ncand;
  for (int i0 = 0; i0 < n; i0++) {
    for (int i1 = i0 + 1; i1 < n; i1++) {
      const DevDetection& a = cand[idx[i0]];
      const DevDetection& b = cand[idx[i1]];
      if (a.id != b.id) continue;
      if (!poly_overlap(a.p, b.p)) continue;
      int pref = 0;
      pref = prefer_smaller(pref, a.hamming, b.hamming);
      pref = prefer_smaller(pref, -a.decision_margin, -b.decision_margin);
      for (int k = 0; k < 3; k++) pref = prefer_smaller(pref, a.H[k], b.H[k]);
      if (pref < 0) {  // keep i0; zarray_remove_index(shuffle=1)
        if (i1 < n - 1) idx[i1] = idx[n - 1];
        n--;
        i1--;
      } else {
        if (i0 < n - 1) idx[i0] = idx[n - 1];
        n--;
        i0--;
        break;
      }
    }
  }
  std::stable_sort(idx, idx + n, [&](int a, int b) { return cand[a].id < cand[b].id; });
  for (int i = 0; i < n && i < cap; i++) write_detection(cand[idx[i]], out + i);
  return n;
}

// The per-batch sequence: frame table H2D, control block reset, the kernels,
// control block + detections D2H (all to/from pinned buffers whose addresses
// never change, so it can be captured once per (nframes, fmt) and replayed).
static hipError_t record_sequence(at_detector* d, int nframes, int fmt, hipStream_t st, hipEvent_t* ev,
                                  const KernelTimer* kt) {
  hipError_t e;
  DevBufs b = d->d;
  b.kt_stage = kt ? kt->stage : -1;  // the timed kernel stamps its device-clock span
  FieldLaunch fl = d->field;
  // (events cannot be recorded between the segments of a split capture; stage profiling launches directly)
  fl.ev[0] = ev ? d->ev_field[0] : nullptr;
  fl.ev[1] = ev ? d->ev_field[1] : nullptr;
  if ((e = launch_pipeline(b, d->g, d->prm, nframes, fmt, d->nblobwg, st, ev, d->st2, d->ev_fork, d->ev_join, kt,
                           d->field_on ? &fl : nullptr)))
    return e;
  // results reach the host zero-copy: k_decode writes the detections into the
  // mapped host buffer and k_pose adds the poses and the control block; without
  // k_pose (tag_size == 0) the control block is copied here
  if (d->prm.tag_size > 0) return hipSuccess;
  return hipMemcpyAsync(d->h_ctrl, d->d_ctrl, d->ctrl_words * 4, hipMemcpyDeviceToHost, st);
}

// KernelTimer::split hook while capturing: close the current segment, open the next
static hipError_t split_capture(void* ctx, int /*which*/) {
  at_detector* d = (at_detector*)ctx;
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(d->st, &g);
  if (e != hipSuccess) return e;
  d->cap_segs.push_back(g);
  return hipStreamBeginCapture(d->st, hipStreamCaptureModeThreadLocal);
}

static hipError_t instantiate(hipGraph_t g, hipGraphExec_t* exec) {
  const hipError_t e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  return e;
}

// Timed kernel under graph replay (bench roofline): segment before it, the kernel,
// segment after it, as three graphs with the timing events recorded between them.
// Not used when the timed kernel sits on the fork branch (its capture spans two
// streams and cannot be cut there): those launch directly.
static int enqueue_split(at_detector* d, int nframes, int fmt) {
  hipStream_t st = d->st;
  const int key = (nframes * 4 + fmt) * 32 + d->kt.stage;
  auto it = d->split_graphs.find(key);
  if (it == d->split_graphs.end()) {
    d->cap_segs.clear();
    KernelTimer kt = d->kt;
    kt.split = split_capture;
    kt.ctx = d;
    HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    hipError_t rec = record_sequence(d, nframes, fmt, st, nullptr, &kt);
    hipGraph_t last = nullptr;
    const hipError_t end = hipStreamEndCapture(st, &last);
    if (last) d->cap_segs.push_back(last);
    if (rec == hipSuccess && end == hipSuccess && d->cap_segs.size() != 3) rec = hipErrorInvalidValue;
    if (rec != hipSuccess || end != hipSuccess) {
      for (auto* g : d->cap_segs) (void)hipGraphDestroy(g);
      d->cap_segs.clear();
      HIPCHK(rec);
      HIPCHK(end);
    }
    at_detector::SplitGraphs sg{};
    hipError_t inst = hipSuccess;
    for (int i = 0; i < 3; i++) {
      const hipError_t r = instantiate(d->cap_segs[i], &sg.seg[i]);
      if (r != hipSuccess && inst == hipSuccess) inst = r;
    }
    d->cap_segs.clear();
    if (inst != hipSuccess) {
      for (auto* g : sg.seg)
        if (g) (void)hipGraphExecDestroy(g);
      HIPCHK(inst);
    }
    it = d->split_graphs.emplace(key, sg).first;
  }
  HIPCHK(hipGraphLaunch(it->second.seg[0], st));
  HIPCHK(hipEventRecord(d->kt.t0, st));
  HIPCHK(hipGraphLaunch(it->second.seg[1], st));
  HIPCHK(hipEventRecord(d->kt.t1, st));
  HIPCHK(hipGraphLaunch(it->second.seg[2], st));
  return AT_OK;
}

static int enqueue(at_detector* d, int nframes, int fmt) {
  hipStream_t st = d->st;
  const bool timed = d->kt.stage >= 0;
  const bool timed_on_fork = timed && d->st2 && (d->kt.stage == 8 || d->kt.stage == 9);
  if (d->profiling || !d->use_graphs || timed_on_fork) {
    HIPCHK(record_sequence(d, nframes, fmt, st, d->profiling ? d->ev_stage : nullptr, timed ? &d->kt : nullptr));
  } else if (timed) {
    const int rc = enqueue_split(d, nframes, fmt);
    if (rc != AT_OK) return rc;
  } else {
    const int key = nframes * 4 + fmt;
    auto it = d->graphs.find(key);
    if (it == d->graphs.end()) {
      hipGraph_t graph = nullptr;
      HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
      const hipError_t rec = record_sequence(d, nframes, fmt, st, nullptr, nullptr);
      const hipError_t end = hipStreamEndCapture(st, &graph);
      HIPCHK(rec);
      HIPCHK(end);
      hipGraphExec_t exec = nullptr;
      HIPCHK(instantiate(graph, &exec));
      it = d->graphs.emplace(key, exec).first;
    }
    HIPCHK(hipGraphLaunch(it->second, st));
  }
  HIPCHK(hipEventRecord(d->ev_done, st));
  d->last_nframes = nframes;
  d->last_fmt = fmt;
  d->last_gray = fmt == AT_FMT_BGR8 || d->prm.taps;  // (YUYV / GRAY8: k_decode samples the frame)
  d->last_sizes = d->g.ctw == 32 || d->prm.taps;     // (throughput mode: the size plane for the taps only)
  d->last_gp = d->prm.gp_c && fmt == AT_FMT_BGR8;
  d->last_mj_color = 0;  // (at_enqueue_mjpg sets it after a colour-on batch)
  d->mj_ent_batch = 0;   // (... and this after a batch decoded by k_mjpg_entropy)
  d->last_field = d->field_on && d->prm.tag_size > 0;
  d->last_und = d->prm.undistort && d->prm.tag_size > 0;
  for (auto& v : d->und_ovf) v.clear();
  d->field_timed = d->last_field && d->profiling;
  d->pending = 1;
  return AT_OK;
}

static double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int collect(at_detector* d, at_detection* out, int cap_per_frame, int* n_per_frame) {
  if (!d->pending) return AT_E_INVALID;
  const double t0 = now_us();
  HIPCHK(hipEventSynchronize(d->ev_done));
  const double t1 = now_us();
  d->host_wait_us += t1 - t0;
  d->pending = 0;
  if (d->profiling) {
    for (int i = 0; i < kNumStages; i++) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, d->ev_stage[i], d->ev_stage[i + 1]));
      d->stage_ms[i] += ms;
    }
    d->stage_batches++;
  }
  if (d->mj_timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, d->ev_mj[0], d->ev_mj[1]));
    d->mj_stats[4] = (uint64_t)((double)ms * 1e6);
    if (d->mj_timed == 2) {
      HIPCHK(hipEventElapsedTime(&ms, d->ev_mj[1], d->ev_mj[2]));
      d->mj_stats[5] = (uint64_t)((double)ms * 1e6);
    }
    d->mj_timed = 0;
  }
  d->field_ns = 0;
  if (d->field_timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, d->ev_field[0], d->ev_field[1]));
    d->field_ns = (uint64_t)((double)ms * 1e6);
    d->field_timed = 0;
  }
  if (d->mj_ent_timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, d->ev_ent[0], d->ev_ent[1]));
    d->mj_stats[6] = (uint64_t)((double)ms * 1e6);
    d->mj_ent_timed = 0;
  }
  if (d->mj_ent_batch) {
    uint32_t most = 0;
    for (int f = 0; f < d->last_nframes; f++) most = std::max(most, d->h_ent_info[(size_t)f * at::kEntInfoWords + 1]);
    d->mj_stats[8] = most;
  }
  if (d->kt.stage >= 0) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, d->kt.t0, d->kt.t1));
    d->kt_ms += ms;
    d->kt_n++;
    uint64_t st[2];
    memcpy(st, d->h_ctrl + d->kstamp_word, sizeof(st));
    st[0] = ~st[0];  // (k_kt_span keeps the complement of the first start: atomicMax on a zeroed word)
    if (st[1] > st[0] && st[0] && d->wclk_khz > 0) {  // (kernels without stamps leave zeros)
      d->kd_ms += (double)(st[1] - st[0]) / d->wclk_khz;
      d->kd_n++;
    }
  }
  const int B = d->B;
  int rc = AT_OK;
  bool bad_entropy = false;
  // each frame's candidates: its slots 0 .. ndets[f] (the first kDetPoolPerFrame
  // already in the host mirror; a frame with more is copied from HBM)
  const int nf = d->last_nframes;
  int* cnt = d->res_n.data();
  // a failed copy leaves no stale counts: every frame reads empty until it is done
  for (int f = 0; f < nf; f++) {
    cnt[f] = 0;
    if (n_per_frame) n_per_frame[f] = 0;
  }
  for (int f = 0; f < nf; f++) {
    const uint32_t status = d->h_ctrl[kCtlStatus * B + f];
    const int ncand = (int)std::min<uint32_t>(d->h_ctrl[kCtlNdets * B + f], kMaxDets);
    int* idx = d->res_idx.data() + (size_t)f * kMaxDets;
    int n = 0;
    if (status & kStatusPairsCapped) rc = AT_E_CAPACITY;  // the first kMaxPairs pairs' detections are kept
    if (d->mj_ent_batch && d->h_ent_info[(size_t)f * at::kEntInfoWords]) {
      bad_entropy = true;  // the frame's entropy-coded data was bad: a flat plane went through, nothing is reported
    } else if (status & (kStatusPairsOverflow | kStatusHashFull | kStatusPointsOverflow | kStatusQuadsOverflow | kStatusDetsOverflow)) {
      rc = AT_E_CAPACITY;
    } else {
      const DevDetection* cand = d->h_dets + (size_t)f * kDetPoolPerFrame;
      if (ncand > kDetPoolPerFrame) {
        std::vector<DevDetection>& v = d->res_ovf[f];
        v.resize(ncand);
        // on the detector's own (non-blocking) stream: a copy on the null stream would
        // serialize with every blocking stream of the process (torch's default stream)
        HIPCHK(hipMemcpyAsync(v.data(), d->d.dets + (size_t)f * kMaxDets, ncand * sizeof(DevDetection),
                              hipMemcpyDeviceToHost, d->st));
        HIPCHK(hipStreamSynchronize(d->st));
        cand = v.data();
      }
      d->res_base[f] = cand;
      for (int i = 0; i < ncand; i++) idx[i] = i;
      n = host_tail(cand, idx, ncand, out ? out + (size_t)f * cap_per_frame : nullptr, out ? cap_per_frame : 0);
    }
    cnt[f] = n;
    if (n_per_frame) n_per_frame[f] = n;
  }
  d->host_tail_us += now_us() - t1;
  return bad_entropy ? AT_E_INVALID : rc;
}

static int check_fmt(int fmt) { return fmt == AT_FMT_YUYV || fmt == AT_FMT_BGR8 || fmt == AT_FMT_GRAY8; }
static size_t frame_bytes(const at_detector* d, int fmt) {
  const size_t npix = (size_t)d->g.W * d->g.H;
  return fmt == AT_FMT_YUYV ? 2 * npix : (fmt == AT_FMT_BGR8 ? 3 * npix : npix);
}

extern "C" {

int at_enqueue_host(at_detector* d, const uint8_t* const* frames, int nframes, at_pixfmt fmt) {
  if (!d || !frames || nframes < 1 || nframes > d->B || !check_fmt(fmt)) return AT_E_INVALID;
  for (int f = 0; f < nframes; f++)
    if (!frames[f]) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));  // the frame table is read by the pending batch
  const size_t fb = frame_bytes(d, fmt);
  // frames back to back in host memory go over in one copy (their staging slots
  // are in_stride apart: one 2-D copy)
  for (int f = 0; f < nframes;) {
    int r = 1;
    while (f + r < nframes && frames[f + r] == frames[f] + (size_t)r * fb) r++;
    uint8_t* dst = d->d_in + (size_t)f * d->in_stride;
    if (r == 1)
      HIPCHK(hipMemcpyAsync(dst, frames[f], fb, hipMemcpyHostToDevice, d->st));
    else
      HIPCHK(hipMemcpy2DAsync(dst, d->in_stride, frames[f], fb, fb, (size_t)r, hipMemcpyHostToDevice, d->st));
    for (int k = 0; k < r; k++) d->h_ftab[f + k] = d->d_in + (size_t)(f + k) * d->in_stride;
    f += r;
  }
  const int rc = enqueue(d, nframes, fmt);
  if (rc) return rc;
  d->last_staged = 1;
  return AT_OK;
}

int at_detect_batch(at_detector* d, const uint8_t* const* frames, int nframes, at_pixfmt fmt, at_detection* out,
                    int cap_per_frame, int* n_per_frame) {
  const int rc = at_enqueue_host(d, frames, nframes, fmt);
  if (rc) return rc;
  return collect(d, out, cap_per_frame, n_per_frame);
}

int at_detect(at_detector* d, const uint8_t* frame, at_pixfmt fmt, at_detection* out, int cap, int* n) {
  const uint8_t* frames[1] = {frame};
  int nn = 0;
  const int rc = at_detect_batch(d, frames, 1, fmt, out, cap, &nn);
  if (n) *n = nn;
  return rc;
}

// ---- MJPG input ---------------------------------------------------------------
// The host parses and entropy-decodes every frame of the batch (at_mjpg.cpp) straight
// into page-locked staging, before anything is waited for or enqueued: a batch still
// running on the GPU is not in the way (its copy read the other staging set), and a bad
// frame leaves the detector as it was.  Then the coefficient streams go to the device,
// k_mjpg_idct writes the GRAY8 planes into the frames' staging slots, and the batch
// continues as host-fed GRAY8 frames (the captured launch sequence is the GRAY8 one).
// With colour on (at_mjpg_set_color) the chroma coefficients travel behind the luma ones
// and two more launches in front of the graph leave each frame's BGR8 image in d_mj_bgr.
// With the device entropy decode on (at_mjpg_set_device_entropy) the host only parses the
// markers: the batch's records (geometry, stream headers, decode tables, raw scan bytes) go
// over in one copy, the slots are zeroed and k_mjpg_entropy writes the dense coefficients in
// front of the same kernels; a frame with more than W * H scan bytes is decoded here as before.
//
// The buffers, allocated on first use.  color: the slots also hold the chroma sub-streams (worst case 4:4:4, all three planes
// dense), and the chroma planes and BGR8 images exist.  Luma-only buffers from earlier
// colour-off batches are replaced (after a pending batch, whose copies read them).
static int mjpg_prepare(at_detector* d, bool color) {
  if (d->d_mj && (!color || d->mj_color_bufs)) return AT_OK;
  const size_t nb = (size_t)(d->g.W / 8) * (d->g.H / 8);
  const size_t slot = ((color ? at::MjpgDecoder::slot_bytes(d->g.W, d->g.H, true) : (size_t)kMjpgHdrBytes + 128 * nb) +
                       255) & ~(size_t)255;
  const size_t total = slot * (size_t)d->B;
  const size_t plane = ((size_t)d->g.W * d->g.H + 255) & ~(size_t)255;
  uint8_t* h[2] = {nullptr, nullptr};
  void *dev = nullptr, *planes = nullptr, *bgr = nullptr;
  if (d->d_mj && d->pending) HIPCHK(hipEventSynchronize(d->ev_done));
  if (hipHostMalloc((void**)&h[0], total, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&h[1], total, hipHostMallocDefault) != hipSuccess ||
      hipMalloc(&dev, total) != hipSuccess ||
      (color && (hipMalloc(&planes, 2 * plane * (size_t)d->B) != hipSuccess ||
                 hipMalloc(&bgr, d->in_stride * (size_t)d->B) != hipSuccess))) {
    if (h[0]) (void)hipHostFree(h[0]);
    if (h[1]) (void)hipHostFree(h[1]);
    if (dev) (void)hipFree(dev);
    if (planes) (void)hipFree(planes);
    return AT_E_NOMEM;
  }
  if (d->d_mj) {  // the luma-only set
    for (auto& a : d->allocs)
      if (a == d->d_mj) a = nullptr;
    (void)hipFree(d->d_mj);
    for (uint8_t*& p : d->mj_host) {
      (void)hipHostFree(p);
      p = nullptr;
    }
  }
  d->allocs.push_back(dev);
  if (color) {
    d->allocs.push_back(planes);
    d->allocs.push_back(bgr);
    d->d_mj_planes = (uint8_t*)planes;
    d->d_mj_bgr = (uint8_t*)bgr;
    d->mj_plane = plane;
    d->mj_color_bufs = 1;
  }
  d->d_mj = (uint8_t*)dev;
  d->mj_host[0] = h[0];
  d->mj_host[1] = h[1];
  d->mj_slot = slot;
  d->mj_cur = 1;
  d->mj_dec.resize(16);  // at_mjpg_set_threads' upper bound
  d->mj_rc.assign((size_t)d->B, 0);
  d->mj_bytes.assign((size_t)d->B, 0);
  d->mj_dense.assign((size_t)d->B, 0);
  return AT_OK;
}

int at_mjpg_set_threads(at_detector* d, int n) {
  if (!d) return AT_E_INVALID;
  d->mj_threads = std::max(1, std::min(16, n));
  return AT_OK;
}

int at_mjpg_set_color(at_detector* d, int enable) {
  if (!d) return AT_E_INVALID;
  d->mj_color = enable ? 1 : 0;
  return AT_OK;
}

int at_mjpg_set_device_entropy(at_detector* d, int enable) {
  if (!d) return AT_E_INVALID;
  d->mj_dev_ent = enable ? 1 : 0;
  return AT_OK;
}

int at_mjpg_set_subseq(at_detector* d, int bytes) {
  if (!d || bytes < 16 || bytes > 256 || (bytes & (bytes - 1))) return AT_E_INVALID;
  d->mj_subseq = bytes;
  return AT_OK;
}

// The buffers of the device entropy decode, allocated on first use: the compressed input (a
// directory of B offsets, then per frame at most a record and W * H scan bytes -- a larger
// frame takes the host route) as two page-locked sets and a device copy, and the kernel's
// scratch for the smallest piece size (16 bytes) and the most blocks a sampling decodes.
static int mjpg_ent_prepare(at_detector* d) {
  if (d->ent.in) return AT_OK;
  const size_t B = (size_t)d->B, npix = (size_t)d->g.W * d->g.H;
  const size_t dir = (B * 8 + 255) & ~(size_t)255;
  const size_t per = (at::kEntRecordMax + npix + 16 + 255) & ~(size_t)255;
  const size_t cap = dir + per * B;
  const uint32_t pieces = (uint32_t)(npix / 16 + 1);
  const uint32_t dcb = (uint32_t)at::ent_max_blocks(d->g.W, d->g.H);
  uint8_t* h[2] = {nullptr, nullptr};
  uint32_t* hinfo = nullptr;
  void* dv[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const size_t sz[6] = {cap, 8 * B * pieces, 8 * B * pieces, 4 * B * pieces, 2 * B * dcb, 4 * B * at::kEntInfoWords};
  bool ok = hipHostMalloc((void**)&h[0], cap, hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&h[1], cap, hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&hinfo, sz[5], hipHostMallocDefault) == hipSuccess;
  for (int i = 0; ok && i < 6; i++) ok = hipMalloc(&dv[i], sz[i]) == hipSuccess;
  if (!ok) {
    for (uint8_t* p : h)
      if (p) (void)hipHostFree(p);
    if (hinfo) (void)hipHostFree(hinfo);
    for (void* p : dv)
      if (p) (void)hipFree(p);
    return AT_E_NOMEM;
  }
  for (void* p : dv) d->allocs.push_back(p);
  memset(hinfo, 0, sz[5]);
  d->mj_ent_host[0] = h[0];
  d->mj_ent_host[1] = h[1];
  d->mj_ent_cap = cap;
  d->h_ent_info = hinfo;
  d->ent.in = (const uint8_t*)dv[0];
  d->ent.entry = (uint64_t*)dv[1];
  d->ent.exit = (uint64_t*)dv[2];
  d->ent.nblk = (uint32_t*)dv[3];
  d->ent.pieces = pieces;
  d->ent.dcdiff = (int16_t*)dv[4];
  d->ent.dc_blocks = dcb;
  d->ent.info = (uint32_t*)dv[5];
  return AT_OK;
}

int at_mjpg_stats(at_detector* d, uint64_t* out, int cap) {
  if (!d || !out || cap < 1) return AT_E_INVALID;
  const int n = std::min(cap, 9);
  for (int i = 0; i < n; i++) out[i] = d->mj_stats[i];
  return n;
}

int at_enqueue_mjpg(at_detector* d, const uint8_t* const* jpgs, const size_t* lens, int nframes, int* bad_frame) {
  if (bad_frame) *bad_frame = -1;
  if (!d || !jpgs || !lens || nframes < 1 || nframes > d->B) return AT_E_INVALID;
  for (int f = 0; f < nframes; f++)
    if (!jpgs[f]) {
      if (bad_frame) *bad_frame = f;
      return AT_E_INVALID;
    }
  HIPCHK(hipSetDevice(d->device));
  const bool color = d->mj_color != 0;
  const int prc = mjpg_prepare(d, color);
  if (prc != AT_OK) return prc;
  const int set = d->mj_cur ^ 1;
  uint8_t* stage = d->mj_host[set];
  const bool dev = d->mj_dev_ent != 0;
  if (dev) {
    const int erc = mjpg_ent_prepare(d);
    if (erc != AT_OK) return erc;
  }
  uint64_t st[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const double t0 = now_us();
  if (dev) {
    // markers only: every frame's record and scan bytes into the staging set, back to back
    // behind the directory; a frame with more than W * H scan bytes is decoded here instead
    uint8_t* es = d->mj_ent_host[set];
    uint64_t* dir = reinterpret_cast<uint64_t*>(es);
    const size_t npix = (size_t)d->g.W * d->g.H;
    size_t at = ((size_t)d->B * 8 + 255) & ~(size_t)255;
    for (int f = 0; f < nframes; f++) {
      size_t scan_pos = 0;
      int rc = at::mjpg_entropy_parse(jpgs[f], lens[f], d->g.W, d->g.H, color, (uint32_t)d->mj_subseq, es + at,
                                      &scan_pos);
      d->mj_dense[(size_t)f] = 0;
      if (rc == AT_OK && lens[f] - scan_pos > npix) {
        at::MjpgDecoder& dec = d->mj_dec[0];
        rc = dec.decode(jpgs[f], lens[f], d->g.W, d->g.H, color);
        if (rc == AT_OK) {
          d->mj_bytes[(size_t)f] = dec.packed_bytes();
          rc = dec.pack(stage + (size_t)f * d->mj_slot, d->mj_slot);
          d->mj_dense[(size_t)f] = dec.dense() ? 1 : 0;
        }
        dir[f] = 0;
        st[7]++;
      } else if (rc == AT_OK) {
        at::EntGeom g;
        memcpy(&g, es + at, sizeof(g));
        const size_t so = at::ent_scan_off(g.ntab);
        memcpy(es + at + so, jpgs[f] + scan_pos, g.scan_len);
        dir[f] = at;
        d->mj_bytes[(size_t)f] = 0;
        at = (at + so + g.scan_len + 15) & ~(size_t)15;
      }
      if (rc != AT_OK) {
        if (bad_frame) *bad_frame = f;
        return rc;  // nothing enqueued, the staging sets in use untouched
      }
    }
    st[3] = (uint64_t)(now_us() - t0);
    if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));  // the frame table and result buffers are reused
    // zero payloads for the kernel to write into, then what crosses the link
    HIPCHK(hipMemsetAsync(d->d_mj, 0, d->mj_slot * (size_t)nframes, d->st));
    HIPCHK(hipMemsetAsync(d->ent.info, 0, sizeof(uint32_t) * at::kEntInfoWords * (size_t)d->B, d->st));
    HIPCHK(hipMemcpyAsync(const_cast<uint8_t*>(d->ent.in), es, at, hipMemcpyHostToDevice, d->st));
    st[1] = at;
    for (int f = 0; f < nframes; f++) {
      st[0] += lens[f];
      st[2] += d->mj_dense[(size_t)f];
      if (!dir[f]) {
        const size_t nbytes = d->mj_bytes[(size_t)f];
        st[1] += nbytes;
        HIPCHK(hipMemcpyAsync(d->d_mj + (size_t)f * d->mj_slot, stage + (size_t)f * d->mj_slot, nbytes,
                              hipMemcpyHostToDevice, d->st));
      }
      d->h_ftab[f] = d->d_in + (size_t)f * d->in_stride;
    }
    const bool etimed = d->profiling != 0;
    if (etimed) {
      for (hipEvent_t& e : d->ev_ent)
        if (!e) HIPCHK(hipEventCreateWithFlags(&e, kTimingEventFlags));
      HIPCHK(hipEventRecord(d->ev_ent[0], d->st));
    }
    at::EntBufs eb = d->ent;
    eb.in_bytes = d->mj_ent_cap;  // (what lies behind the bytes copied is never a frame's: its lengths bound it)
    eb.coef = d->d_mj;
    eb.slot = d->mj_slot;
    eb.nb = (uint32_t)(d->g.W / 8) * (uint32_t)(d->g.H / 8);
    HIPCHK(launch_mjpg_entropy(eb, nframes, d->st));
    if (etimed) HIPCHK(hipEventRecord(d->ev_ent[1], d->st));
    d->mj_ent_timed = etimed ? 1 : 0;
    HIPCHK(hipMemcpyAsync(d->h_ent_info, d->ent.info, sizeof(uint32_t) * at::kEntInfoWords * (size_t)nframes,
                          hipMemcpyDeviceToHost, d->st));
  } else {
    const int nthr = std::min(d->mj_threads, nframes);
    auto work = [&](int t) {
      at::MjpgDecoder& dec = d->mj_dec[(size_t)t];
      for (int f = t; f < nframes; f += nthr) {
        int rc = dec.decode(jpgs[f], lens[f], d->g.W, d->g.H, color);
        if (rc == AT_OK) {
          d->mj_bytes[(size_t)f] = dec.packed_bytes();
          rc = dec.pack(stage + (size_t)f * d->mj_slot, d->mj_slot);
          d->mj_dense[(size_t)f] = dec.dense() ? 1 : 0;
        }
        d->mj_rc[(size_t)f] = rc;
      }
    };
    if (nthr > 1) {
      std::vector<std::thread> pool;
      for (int t = 1; t < nthr; t++) pool.emplace_back(work, t);
      work(0);
      for (auto& th : pool) th.join();
    } else {
      work(0);
    }
    const double t1 = now_us();
    for (int f = 0; f < nframes; f++)
      if (d->mj_rc[(size_t)f] != AT_OK) {
        if (bad_frame) *bad_frame = f;
        return d->mj_rc[(size_t)f];  // nothing enqueued, the staging set in use untouched
      }
    if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));  // the frame table and result buffers are reused
    st[3] = (uint64_t)(t1 - t0);
    for (int f = 0; f < nframes; f++) {
      const size_t nbytes = d->mj_bytes[(size_t)f];
      st[0] += lens[f];
      st[1] += nbytes;
      st[2] += d->mj_dense[(size_t)f];
      HIPCHK(hipMemcpyAsync(d->d_mj + (size_t)f * d->mj_slot, stage + (size_t)f * d->mj_slot, nbytes,
                            hipMemcpyHostToDevice, d->st));
      d->h_ftab[f] = d->d_in + (size_t)f * d->in_stride;
    }
  }
  d->mj_cur = set;
  const bool timed = d->profiling != 0;
  if (timed) {
    for (hipEvent_t& e : d->ev_mj)
      if (!e) HIPCHK(hipEventCreateWithFlags(&e, kTimingEventFlags));
    HIPCHK(hipEventRecord(d->ev_mj[0], d->st));
  }
  HIPCHK(launch_mjpg_idct(d->d_mj, d->mj_slot, d->d_in, d->in_stride, d->g.W, d->g.H, nframes, d->st));
  if (timed) HIPCHK(hipEventRecord(d->ev_mj[1], d->st));
  if (color) {
    // the chroma planes and the BGR8 images, then the game-piece tensors from those
    HIPCHK(launch_mjpg_color(d->d_mj, d->mj_slot, d->d_in, d->d_mj_planes, d->mj_plane, d->d_mj_bgr, d->in_stride,
                             d->g.W, d->g.H, nframes, d->st));
    if (timed) HIPCHK(hipEventRecord(d->ev_mj[2], d->st));
    if (d->prm.gp_c)
      for (int f = 0; f < nframes; f++)
        HIPCHK(launch_gp_preprocess(d->d_mj_bgr + (size_t)f * d->in_stride, d->g.W, d->g.H,
                                    d->d.gp_out + (size_t)f * d->prm.gp_c * d->prm.gp_w * d->prm.gp_h, d->prm.gp_w,
                                    d->prm.gp_h, d->prm.gp_c, d->st));
  }
  d->mj_timed = timed ? (color ? 2 : 1) : 0;
  const int rc = enqueue(d, nframes, AT_FMT_GRAY8);
  if (rc) return rc;
  d->last_staged = 1;
  d->last_mj_color = color;
  d->last_gp = color && d->prm.gp_c;
  d->mj_ent_batch = dev;
  memcpy(d->mj_stats, st, sizeof(st));
  return AT_OK;
}

int at_mjpg_bgr(at_detector* d, int frame, const uint8_t** dev_ptr) {
  if (!d || !dev_ptr || !d->last_mj_color || frame < 0 || frame >= d->last_nframes) return AT_E_INVALID;
  *dev_ptr = d->d_mj_bgr + (size_t)frame * d->in_stride;
  return AT_OK;
}

int at_mjpg_copy_bgr(at_detector* d, int frame, uint8_t* dst, size_t cap) {
  const uint8_t* src = nullptr;
  const int rc = at_mjpg_bgr(d, frame, &src);
  if (rc != AT_OK) return rc;
  const size_t n = (size_t)d->g.W * d->g.H * 3;
  if (!dst || cap < n) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));
  // on the detector's own stream (no null-stream copy), in order behind k_mjpg_bgr
  HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, d->st));
  HIPCHK(hipStreamSynchronize(d->st));
  return AT_OK;
}

int at_detect_mjpg_batch(at_detector* d, const uint8_t* const* jpgs, const size_t* lens, int nframes,
                         at_detection* out, int cap_per_frame, int* n_per_frame, int* bad_frame) {
  const int rc = at_enqueue_mjpg(d, jpgs, lens, nframes, bad_frame);
  if (rc) return rc;
  return collect(d, out, cap_per_frame, n_per_frame);
}

int at_detect_mjpg(at_detector* d, const uint8_t* jpg, size_t len, at_detection* out, int cap, int* n) {
  const uint8_t* jpgs[1] = {jpg};
  const size_t lens[1] = {len};
  int nn = 0;
  const int rc = at_detect_mjpg_batch(d, jpgs, lens, 1, out, cap, &nn, nullptr);
  if (n) *n = nn;
  return rc;
}

int at_enqueue_device(at_detector* d, const void* d_frames, size_t frame_stride, int nframes, at_pixfmt fmt) {
  if (!d || !d_frames || nframes < 1 || nframes > d->B || !check_fmt(fmt)) return AT_E_INVALID;
  if (fmt == AT_FMT_YUYV && frame_stride % 16) return AT_E_INVALID;
  if (frame_stride % 8) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));  // pinned buffers are reused
  for (int f = 0; f < nframes; f++) d->h_ftab[f] = (const uint8_t*)d_frames + (size_t)f * frame_stride;
  const int rc = enqueue(d, nframes, fmt);
  d->last_staged = 0;
  return rc;
}

int at_stream_wait(at_detector* d, void* stream) {
  if (!d) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipEventRecord(d->ev_ext, (hipStream_t)stream));
  HIPCHK(hipStreamWaitEvent(d->st, d->ev_ext, 0));
  return AT_OK;
}

int at_collect(at_detector* d, at_detection* out, int cap_per_frame, int* n_per_frame) {
  if (!d) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  return collect(d, out, cap_per_frame, n_per_frame);
}

int at_detect_device(at_detector* d, const void* d_frames, size_t frame_stride, int nframes, at_pixfmt fmt,
                     at_detection* out, int cap_per_frame, int* n_per_frame) {
  int rc = at_enqueue_device(d, d_frames, frame_stride, nframes, fmt);
  if (rc) return rc;
  return at_collect(d, out, cap_per_frame, n_per_frame);
}

int at_set_profiling(at_detector* d, int enable) {
  if (!d) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));
  if (enable && !d->ev_stage[0])
    for (int i = 0; i <= kNumStages; i++) HIPCHK(hipEventCreateWithFlags(&d->ev_stage[i], kTimingEventFlags));
  d->profiling = enable ? 1 : 0;
  for (int i = 0; i < kNumStages; i++) d->stage_ms[i] = 0;
  d->stage_batches = 0;
  return AT_OK;
}

int at_stage_times(at_detector* d, double* ms, int cap) {
  if (!d || !ms || cap < kNumStages + 1) return AT_E_INVALID;
  for (int i = 0; i < kNumStages; i++) ms[i] = d->stage_batches ? d->stage_ms[i] / d->stage_batches : 0.0;
  ms[kNumStages] = (double)d->stage_batches;
  return kNumStages;
}

const char* at_stage_name(int stage) {
  return (stage >= 0 && stage < kNumStages) ? kStageNames[stage] : "";
}

int at_set_kernel_timer(at_detector* d, int stage) {
  if (!d || stage < -1 || stage >= kNumStages) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));
  d->kt.stage = stage;
  d->kt_ms = 0;
  d->kt_n = 0;
  d->kd_ms = 0;
  d->kd_n = 0;
  return AT_OK;
}

int at_kernel_time(at_detector* d, double* avg_ms, long long* launches) {
  if (!d || !avg_ms) return AT_E_INVALID;
  *avg_ms = d->kt_n ? d->kt_ms / (double)d->kt_n : 0.0;
  if (launches) *launches = d->kt_n;
  return AT_OK;
}

int at_kernel_span(at_detector* d, double* avg_ms, long long* launches) {
  if (!d || !avg_ms) return AT_E_INVALID;
  *avg_ms = d->kd_n ? d->kd_ms / (double)d->kd_n : 0.0;
  if (launches) *launches = d->kd_n;
  return AT_OK;
}

int at_batch_stats(at_detector* d, uint64_t* out, int cap) {
  if (!d || !out || cap < 1) return AT_E_INVALID;
  if (d->pending) return AT_E_INVALID;
  const int B = d->B;
  uint64_t v[12] = {0};
  v[0] = (uint64_t)d->last_nframes;
  for (int f = 0; f < d->last_nframes; f++) {
    v[1] += d->h_ctrl[kCtlNpts * B + f];
    v[2] += d->h_ctrl[kCtlNpairs * B + f];
    v[6] += d->h_ctrl[kCtlNdets * B + f];
    v[9] += d->h_ctrl[kCtlNlr * B + f];
    v[10] = std::max<uint64_t>(v[10], d->h_ctrl[kCtlNlr * B + f]);
    v[11] += d->h_ctrl[kCtlCclOvf * B + f] != 0;
  }
  v[5] = d->h_ctrl[kCtlNquads * B];  // FitQuads records of the batch (counted per blob team)
  v[3] = d->h_ctrl[kCtlPerFrame * B + kCtlBlobPts];
  v[4] = d->h_ctrl[kCtlPerFrame * B + kCtlBlobPts + 1];
  v[7] = (uint64_t)d->host_wait_us;
  v[8] = (uint64_t)d->host_tail_us;
  const int n = std::min(cap, 12);
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}

int at_poses(at_detector* d, int frame, at_pose* out, int cap) {
  if (!d || frame < 0 || frame >= d->last_nframes || (cap > 0 && !out)) return AT_E_INVALID;
  if (d->pending) return AT_E_INVALID;  // collect first
  if (!(d->prm.tag_size > 0)) return 0;
  const int n = d->res_n[frame];
  for (int i = 0; i < n && i < cap; i++) {
    const DevDetection& v = d->res_base[frame][d->res_idx[(size_t)frame * kMaxDets + i]];
    at_pose& p = out[i];
    p.id = v.id;
    memcpy(p.R, v.pose_R, sizeof(p.R));
    memcpy(p.t, v.pose_t, sizeof(p.t));
    p.err = v.pose_err[0] <= v.pose_err[1] ? v.pose_err[0] : v.pose_err[1];  // estimate_tag_pose
  }
  return n;
}

int at_detections(at_detector* d, int frame, at_detection* out, int cap) {
  if (!d || frame < 0 || frame >= d->last_nframes || (cap > 0 && !out)) return AT_E_INVALID;
  if (d->pending) return AT_E_INVALID;
  const int n = d->res_n[frame];
  for (int i = 0; i < n && i < cap; i++)
    write_detection(d->res_base[frame][d->res_idx[(size_t)frame * kMaxDets + i]], out + i);
  return n;
}

int at_max_detections(void) { return kMaxDets; }

int at_tag_detections(const at_pose* poses, int n, const double* extr_R, const double* extr_t,
                      at_tag_detection* out) {
  if (n < 0 || (n > 0 && (!poses || !out))) return AT_E_INVALID;
  static const double kEye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, kZero[3] = {0, 0, 0};
  const double* Re = extr_R ? extr_R : kEye;
  const double* te = extr_t ? extr_t : kZero;
  std::vector<at_tag_detection> v((size_t)n);
  for (int i = 0; i < n; i++) {
    at_tag_detection& o = v[i];
    o.id = poses[i].id;
    for (int k = 0; k < 3; k++) o.camera[k] = poses[i].t[k];
    for (int r = 0; r < 3; r++)  // extrinsic_rotation_ * camera_point_mat + extrinsic_offset_
      o.robot[r] = Re[r * 3 + 0] * o.camera[0] + Re[r * 3 + 1] * o.camera[1] + Re[r * 3 + 2] * o.camera[2] + te[r];
    o.distance = std::sqrt(o.camera[0] * o.camera[0] + o.camera[1] * o.camera[1] + o.camera[2] * o.camera[2]);
    o.err = poses[i].err;
  }
  std::stable_sort(v.begin(), v.end(),
                   [](const at_tag_detection& a, const at_tag_detection& b) { return a.distance < b.distance; });
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}

// ---- annotated image ------------------------------------
// (outline_prims, the segments of node/at_node.cpp's draw_detection_outlines: at_preview.cpp)

// segments drawn onto `bgr` on the detector's stream (not waited for)
// (dw x dh: the image's size, the detector's geometry or a preview's inside it; 0: the detector's)
static int draw_prims(at_detector* d, const std::vector<DrawPrim>& prims, uint8_t* bgr, int dw = 0, int dh = 0) {
  HIPCHK(hipSetDevice(d->device));
  if (prims.empty()) return AT_OK;
  const size_t W = dw ? (size_t)dw : (size_t)d->g.W, H = dh ? (size_t)dh : (size_t)d->g.H;
  if (!d->d_last) {
    const size_t full = (size_t)d->g.W * d->g.H;
    HIPCHK(hipMalloc((void**)&d->d_last, full * 4));
    HIPCHK(hipMemset(d->d_last, 0, full * 4));  // kept zero by the paint pass
  }
  if (prims.size() > d->prims_cap) {
    if (d->d_prims) HIPCHK(hipFree(d->d_prims));
    d->d_prims = nullptr;
    d->prims_cap = 0;
    const size_t cap = std::max<size_t>(1024, prims.size() * 2);
    HIPCHK(hipMalloc((void**)&d->d_prims, cap * sizeof(DrawPrim)));
    d->prims_cap = cap;
  }
  HIPCHK(hipMemcpyAsync(d->d_prims, prims.data(), prims.size() * sizeof(DrawPrim), hipMemcpyHostToDevice, d->st));
  HIPCHK(launch_draw(d->d_prims, (int)prims.size(), d->d_last, bgr, (int)W, (int)H, d->st));
  return AT_OK;
}

// the outline segments drawn onto `bgr` on the detector's stream (not waited for)
static int draw_outlines(at_detector* d, const at_detection* dets, int n, uint8_t* bgr) {
  if (!d || n < 0 || (n > 0 && !dets) || !bgr) return AT_E_INVALID;
  std::vector<DrawPrim> prims;
  outline_prims(dets, n, &prims);
  return draw_prims(d, prims, bgr);
}

int at_draw_outlines_device(at_detector* d, const at_detection* dets, int n, uint8_t* bgr) {
  const int rc = draw_outlines(d, dets, n, bgr);
  if (rc != AT_OK) return rc;
  HIPCHK(hipStreamSynchronize(d->st));
  return AT_OK;
}

int at_annotate_staged(at_detector* d, int frame, const at_detection* dets, int n, uint8_t* bgr_out) {
  if (!d || !bgr_out || n < 0 || (n > 0 && !dets)) return AT_E_INVALID;
  if (!d->last_staged || (d->last_fmt != AT_FMT_BGR8 && !d->last_mj_color) || frame < 0 || frame >= d->last_nframes)
    return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));
  // a colour MJPG batch: the frame's decoded image (its d_in slot holds the gray plane)
  uint8_t* img = (d->last_mj_color ? d->d_mj_bgr : d->d_in) + (size_t)frame * d->in_stride;
  const int rc = draw_outlines(d, dets, n, img);
  if (rc != AT_OK) return rc;
  // in stream order after the drawing, on the detector's stream (no null-stream copy);
  // DMA straight into a page-locked bgr_out (at_host_alloc)
  HIPCHK(hipMemcpyAsync(bgr_out, img, (size_t)d->g.W * d->g.H * 3, hipMemcpyDeviceToHost, d->st));
  HIPCHK(hipStreamSynchronize(d->st));
  return AT_OK;
}

// ---- game-piece output parse ------------------------------------------------------
// k_gp_cand + k_gp_nms on the detector's stream (outside the captured graphs), behind an
// event of the producer's stream; the kernels leave boxes and counts in mapped page-locked
// memory, the host waits for the stream and copies them to the caller.
static_assert(sizeof(at_gp_box) == sizeof(GpBox), "at_gp.h carries the ABI's box");

static int gp_prepare(at_detector* d) {
  if (d->gp.cnt) return AT_OK;
  const size_t B = (size_t)d->B;
  void *cnt = nullptr, *key = nullptr, *cls = nullptr;
  GpBox* out = nullptr;
  uint32_t* info = nullptr;
  if (hipMalloc(&cnt, B * kGpCntStride * 4) != hipSuccess || hipMalloc(&key, B * kGpMaxCand * 8) != hipSuccess ||
      hipMalloc(&cls, B * kGpMaxCand * 4) != hipSuccess ||
      hipHostMalloc((void**)&out, B * kGpMaxCand * sizeof(GpBox), hipHostMallocMapped) != hipSuccess ||
      hipHostMalloc((void**)&info, B * 2 * 4, hipHostMallocMapped) != hipSuccess) {
    for (void* p : {cnt, key, cls})
      if (p) (void)hipFree(p);
    if (out) (void)hipHostFree(out);
    if (info) (void)hipHostFree(info);
    return AT_E_NOMEM;
  }
  for (void* p : {cnt, key, cls}) d->allocs.push_back(p);
  d->h_gp_out = out;
  d->h_gp_info = info;
  memset(info, 0, B * 2 * 4);
  HIPCHK(hipMemset(cnt, 0, B * kGpCntStride * 4));  // from here on k_gp_nms leaves every counter it read at 0
  HIPCHK(hipHostGetDevicePointer((void**)&d->gp.out, out, 0));
  HIPCHK(hipHostGetDevicePointer((void**)&d->gp.info, info, 0));
  d->gp.key = (uint64_t*)key;
  d->gp.cls = (int32_t*)cls;
  d->gp.cnt = (uint32_t*)cnt;
  return AT_OK;
}

static int gp_parse_run(at_detector* d, const float* d_raw, size_t frame_stride, int nframes, int num_predictions,
                        int num_classes, float conf_thr, float iou_thr, int model_w, int model_h,
                        void* producer_stream, at_gp_box* out, int cap_per_frame, int* n_per_frame,
                        int* status_per_frame);

int at_gp_parse_device(at_detector* d, const float* d_raw, size_t frame_stride, int nframes, int num_predictions,
                       int num_classes, float conf_thr, float iou_thr, int model_w, int model_h,
                       void* producer_stream, at_gp_box* out, int cap_per_frame, int* n_per_frame,
                       int* status_per_frame) {
  if (!d || !d_raw || !n_per_frame || cap_per_frame < 0 || (cap_per_frame > 0 && !out)) return AT_E_INVALID;
  if (num_predictions < 1 || num_classes < 1 || nframes < 1 || nframes > d->B || !std::isfinite(conf_thr) ||
      !std::isfinite(iou_thr) || model_w < 1 || model_h < 1)
    return AT_E_INVALID;
  if (frame_stride < ((size_t)num_classes + 4) * (size_t)num_predictions) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  const int prc = gp_prepare(d);
  if (prc != AT_OK) return prc;
  const int rc = gp_parse_run(d, d_raw, frame_stride, nframes, num_predictions, num_classes, conf_thr, iou_thr,
                              model_w, model_h, producer_stream, out, cap_per_frame, n_per_frame, status_per_frame);
  if (rc != AT_OK) {
    // k_gp_cand may have counted without k_gp_nms zeroing after it: the next call must not start from that
    (void)hipStreamSynchronize(d->st);
    (void)hipMemset(d->gp.cnt, 0, (size_t)d->B * kGpCntStride * 4);
  }
  return rc;
}

// the launches, the wait and the copy-out of at_gp_parse_device (arguments checked, buffers there)
static int gp_parse_run(at_detector* d, const float* d_raw, size_t frame_stride, int nframes, int num_predictions,
                        int num_classes, float conf_thr, float iou_thr, int model_w, int model_h,
                        void* producer_stream, at_gp_box* out, int cap_per_frame, int* n_per_frame,
                        int* status_per_frame) {
  HIPCHK(hipEventRecord(d->ev_ext, (hipStream_t)producer_stream));
  HIPCHK(hipStreamWaitEvent(d->st, d->ev_ext, 0));
  const bool timed = d->profiling != 0;
  if (timed) {
    for (hipEvent_t& e : d->ev_gp)
      if (!e) HIPCHK(hipEventCreateWithFlags(&e, kTimingEventFlags));
    HIPCHK(hipEventRecord(d->ev_gp[0], d->st));
  }
  HIPCHK(launch_gp_parse(d_raw, frame_stride, nframes, num_predictions, num_classes, conf_thr, iou_thr,
                         gp_scale(d->g.W, model_w), gp_scale(d->g.H, model_h), d->gp, d->st));
  if (timed) HIPCHK(hipEventRecord(d->ev_gp[1], d->st));
  HIPCHK(hipStreamSynchronize(d->st));
  uint64_t cand_sum = 0, cand_max = 0, kept_sum = 0;
  for (int f = 0; f < nframes; f++) {
    const volatile uint32_t* info = d->h_gp_info + 2 * f;
    const uint32_t kept = info[0], cand = info[1];
    if (kept > (uint32_t)kGpMaxCand) return AT_E_HIP;  // (cannot happen: at most one box per candidate)
    cand_sum += cand;
    cand_max = std::max<uint64_t>(cand_max, cand);
    kept_sum += kept;
    n_per_frame[f] = (int)kept;
    if (status_per_frame) status_per_frame[f] = cand > (uint32_t)kGpMaxCand ? AT_E_CAPACITY : AT_OK;
    const size_t nw = std::min<size_t>(kept, (size_t)cap_per_frame);
    if (nw) memcpy(out + (size_t)f * cap_per_frame, d->h_gp_out + (size_t)f * kGpMaxCand, nw * sizeof(GpBox));
  }
  d->gp_stats[0] = cand_sum;
  d->gp_stats[1] = cand_max;
  d->gp_stats[2] = kept_sum;
  d->gp_stats[3] = 0;
  if (timed) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, d->ev_gp[0], d->ev_gp[1]));
    d->gp_stats[3] = (uint64_t)((double)ms * 1e6);
  }
  return AT_OK;
}

int at_gp_parse_stats(at_detector* d, uint64_t* out, int cap) {
  if (!d || !out || cap < 1) return AT_E_INVALID;
  const int n = std::min(cap, 4);
  for (int i = 0; i < n; i++) out[i] = d->gp_stats[i];
  return n;
}

// (box_prims, the rectangle as four 2-px segments in the class colour: at_preview.cpp)

int at_gp_draw_boxes_device(at_detector* d, const at_gp_box* boxes, int n, uint8_t* bgr) {
  if (!d || n < 0 || (n > 0 && !boxes) || !bgr) return AT_E_INVALID;
  std::vector<DrawPrim> prims;
  box_prims(d->g.W, d->g.H, boxes, n, &prims);
  const int rc = draw_prims(d, prims, bgr);
  if (rc != AT_OK) return rc;
  HIPCHK(hipStreamSynchronize(d->st));
  return AT_OK;
}

// the staged image of frame `frame` of the last batch, as at_annotate_staged gates it
static int gp_staged_image(at_detector* d, int frame, uint8_t** img) {
  if (!d->last_staged || (d->last_fmt != AT_FMT_BGR8 && !d->last_mj_color) || frame < 0 || frame >= d->last_nframes)
    return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));
  *img = (d->last_mj_color ? d->d_mj_bgr : d->d_in) + (size_t)frame * d->in_stride;
  return AT_OK;
}

int at_gp_annotate_staged(at_detector* d, int frame, const at_gp_box* boxes, int n, uint8_t* bgr_out) {
  if (!d || !bgr_out || n < 0 || (n > 0 && !boxes)) return AT_E_INVALID;
  uint8_t* img = nullptr;
  int rc = gp_staged_image(d, frame, &img);
  if (rc != AT_OK) return rc;
  std::vector<DrawPrim> prims;
  box_prims(d->g.W, d->g.H, boxes, n, &prims);
  rc = draw_prims(d, prims, img);
  if (rc != AT_OK) return rc;
  HIPCHK(hipMemcpyAsync(bgr_out, img, (size_t)d->g.W * d->g.H * 3, hipMemcpyDeviceToHost, d->st));
  HIPCHK(hipStreamSynchronize(d->st));
  return AT_OK;
}

int at_gp_copy_raw(at_detector* d, const float* d_raw, float* dst, size_t count) {
  if (!d || !d_raw || !dst) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipMemcpyAsync(dst, d_raw, count * sizeof(float), hipMemcpyDeviceToHost, d->st));
  HIPCHK(hipStreamSynchronize(d->st));
  return AT_OK;
}

// ---- JPEG output ----------------------------------------------------------------
// The annotated image leaves the GPU as a finished baseline JPEG (k_jpg_fdct, the four
// entropy-coding launches, k_jpg_pack on the detector's stream, outside the captured graphs).  The header is written
// by the host; k_jpg_pack leaves the length of what follows it in a mapped host word, the
// host waits for the stream, checks the capacity and copies exactly those bytes.
static int jpeg_prepare(at_detector* d) {
  if (d->jpg.coef) return AT_OK;
  size_t coef_b = 0, bits_w = 0, out_b = 0, rows = 0;
  for (int s : {kJpg420, kJpg422, kJpg444}) {
    JpgGeom g;
    if (!jpg_geom(d->g.W, d->g.H, s, &g)) return AT_E_INVALID;  // wider or taller than a JPEG can be
    const size_t nbr = (size_t)g.mcux * g.bpm;
    coef_b = std::max(coef_b, nbr * g.mcuy * 128);
    bits_w = std::max(bits_w, (nbr * (kJpgBlockBytes / 4) + 4) * g.mcuy);
    out_b = std::max(out_b, jpg_max_bytes(d->g.W, d->g.H, s) - kJpgHeaderMax);
    rows = std::max(rows, (size_t)g.mcuy);
  }
  uint32_t tab[kJpgTabWords];
  jpg_huff_tables(tab);
  void *coef = nullptr, *dtab = nullptr, *bits = nullptr, *rowv = nullptr, *out = nullptr, *blen = nullptr;
  uint32_t* total = nullptr;
  if (hipMalloc(&coef, coef_b) != hipSuccess || hipMalloc(&dtab, sizeof(tab)) != hipSuccess ||
      hipMalloc(&bits, bits_w * 4) != hipSuccess || hipMalloc(&rowv, 2 * rows * 4) != hipSuccess ||
      hipMalloc(&out, out_b) != hipSuccess || hipMalloc(&blen, coef_b / 128 * 4) != hipSuccess ||
      hipHostMalloc((void**)&total, 64, hipHostMallocMapped) != hipSuccess) {
    for (void* p : {coef, dtab, bits, rowv, out, blen})
      if (p) (void)hipFree(p);
    return AT_E_NOMEM;
  }
  for (void* p : {coef, dtab, bits, rowv, out, blen}) d->allocs.push_back(p);
  d->h_jpg_total = total;
  *total = 0;
  HIPCHK(hipMemcpy(dtab, tab, sizeof(tab), hipMemcpyHostToDevice));
  HIPCHK(hipHostGetDevicePointer((void**)&d->jpg.total, total, 0));
  d->jpg.tab = (const uint32_t*)dtab;
  d->jpg.bits = (uint32_t*)bits;
  d->jpg.blen = (uint32_t*)blen;
  d->jpg.row_raw = (uint32_t*)rowv;
  d->jpg.row_len = (uint32_t*)rowv + rows;
  d->jpg.out = (uint8_t*)out;
  d->jpg_out_cap = out_b;
  d->jpg.coef = (int16_t*)coef;
  return AT_OK;
}

// `img` (device, the detector's geometry) encoded on the detector's stream behind what is
// queued there; returns when the bytes are in `out`
// (ew x eh: the image's size, the detector's geometry or a preview's inside it; 0: the detector's)
static int encode_jpeg(at_detector* d, const uint8_t* img, int quality, int sampling, uint8_t* out, size_t cap,
                       size_t* len, int ew = 0, int eh = 0) {
  JpgGeom g;
  const int W = ew ? ew : d->g.W, H = eh ? eh : d->g.H;
  if (W > d->g.W || H > d->g.H) return AT_E_INVALID;  // the buffers of jpeg_prepare bound it
  if (quality < 1 || quality > 100 || !jpg_geom(W, H, sampling, &g) || ((uintptr_t)img & 7))
    return AT_E_INVALID;
  const int prc = jpeg_prepare(d);
  if (prc != AT_OK) return prc;
  if (!d->jpg_hdr_len || d->jpg_hdr_q != quality || d->jpg_hdr_s != sampling || d->jpg_hdr_w != W ||
      d->jpg_hdr_h != H) {
    d->jpg_hdr_len = jpg_write_header(d->jpg_hdr, W, H, quality, sampling);
    d->jpg_hdr_q = quality;
    d->jpg_hdr_s = sampling;
    d->jpg_hdr_w = W;
    d->jpg_hdr_h = H;
  }
  d->jpg.row_words = (size_t)g.mcux * g.bpm * (kJpgBlockBytes / 4) + 4;
  const bool timed = d->profiling != 0;
  if (timed) {
    for (hipEvent_t& e : d->ev_jpg)
      if (!e) HIPCHK(hipEventCreateWithFlags(&e, kTimingEventFlags));
    HIPCHK(hipEventRecord(d->ev_jpg[0], d->st));
  }
  HIPCHK(launch_jpg_encode(img, W, H, quality, sampling, d->jpg, d->st));
  if (timed) HIPCHK(hipEventRecord(d->ev_jpg[1], d->st));
  HIPCHK(hipStreamSynchronize(d->st));
  const size_t body = *(volatile uint32_t*)d->h_jpg_total;
  if (body > d->jpg_out_cap) return AT_E_HIP;  // (cannot happen: the buffers hold the worst case)
  const size_t need = d->jpg_hdr_len + body;
  *len = need;
  d->jpg_stats[0] = need;
  d->jpg_stats[1] = 0;
  if (timed) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, d->ev_jpg[0], d->ev_jpg[1]));
    d->jpg_stats[1] = (uint64_t)((double)ms * 1e6);
  }
  if (need > cap) return AT_E_CAPACITY;
  memcpy(out, d->jpg_hdr, d->jpg_hdr_len);
  // DMA straight into a page-locked `out` (at_host_alloc)
  HIPCHK(hipMemcpyAsync(out + d->jpg_hdr_len, d->jpg.out, body, hipMemcpyDeviceToHost, d->st));
  HIPCHK(hipStreamSynchronize(d->st));
  return AT_OK;
}

int at_encode_jpeg_device(at_detector* d, const uint8_t* bgr, int quality, int sampling, uint8_t* out, size_t cap,
                          size_t* len) {
  if (len) *len = 0;
  if (!d || !bgr || !out || !len) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  return encode_jpeg(d, bgr, quality, sampling, out, cap, len);
}

int at_annotate_jpeg(at_detector* d, int frame, const at_detection* dets, int n, int quality, int sampling,
                     uint8_t* out, size_t cap, size_t* len) {
  if (len) *len = 0;
  if (!d || !out || !len || n < 0 || (n > 0 && !dets)) return AT_E_INVALID;
  if (!d->last_staged || (d->last_fmt != AT_FMT_BGR8 && !d->last_mj_color) || frame < 0 || frame >= d->last_nframes)
    return AT_E_INVALID;
  JpgGeom g;
  if (quality < 1 || quality > 100 || !jpg_geom(d->g.W, d->g.H, sampling, &g)) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));
  uint8_t* img = (d->last_mj_color ? d->d_mj_bgr : d->d_in) + (size_t)frame * d->in_stride;
  const int rc = draw_outlines(d, dets, n, img);
  if (rc != AT_OK) return rc;
  return encode_jpeg(d, img, quality, sampling, out, cap, len);
}

int at_gp_annotate_jpeg(at_detector* d, int frame, const at_gp_box* boxes, int n, int quality, int sampling,
                        uint8_t* out, size_t cap, size_t* len) {
  if (len) *len = 0;
  if (!d || !out || !len || n < 0 || (n > 0 && !boxes)) return AT_E_INVALID;
  JpgGeom g;
  if (quality < 1 || quality > 100 || !jpg_geom(d->g.W, d->g.H, sampling, &g)) return AT_E_INVALID;
  uint8_t* img = nullptr;
  int rc = gp_staged_image(d, frame, &img);
  if (rc != AT_OK) return rc;
  std::vector<DrawPrim> prims;
  box_prims(d->g.W, d->g.H, boxes, n, &prims);
  rc = draw_prims(d, prims, img);
  if (rc != AT_OK) return rc;
  return encode_jpeg(d, img, quality, sampling, out, cap, len);
}

int at_jpeg_stats(at_detector* d, uint64_t* out, int cap) {
  if (!d || !out || cap < 1) return AT_E_INVALID;
  const int n = std::min(cap, 2);
  for (int i = 0; i < n; i++) out[i] = d->jpg_stats[i];
  return n;
}

// ---- preview stream -------------------------------------------------------------
// k_preview turns a staged frame of any format into the pw x ph BGR8 image d_pv (the source
// is only read), the existing draw and encode kernels run on it at that geometry, and a
// bounded quality search (preview_budget_search, shared with the CPU reference) keeps the
// stream under a byte budget.  On the detector's stream, outside the captured graphs.

// the frame a host-fed batch staged: any format, MJPG with or without colour
static int preview_source(at_detector* d, int frame, const uint8_t** src, int* fmt) {
  if (!d->last_staged || frame < 0 || frame >= d->last_nframes) return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  if (d->pending) HIPCHK(hipEventSynchronize(d->ev_done));
  // a colour MJPG batch: the decoded image; a luma-only one: the gray plane in the frame's slot
  *src = (d->last_mj_color ? d->d_mj_bgr : d->d_in) + (size_t)frame * d->in_stride;
  *fmt = d->last_mj_color ? (int)AT_FMT_BGR8 : d->last_fmt;
  return AT_OK;
}

// d_pv = the annotated preview of `src`, queued on the detector's stream (not waited for)
static int preview_draw(at_detector* d, const uint8_t* src, int fmt, const PvGeom& g, const at_detection* dets, int n,
                        const at_gp_box* boxes, int nb) {
  if (!d->d_pv) HIPCHK(hipMalloc((void**)&d->d_pv, (size_t)d->g.W * d->g.H * 3));
  memset(d->pv_stats, 0, sizeof(d->pv_stats));
  d->pv_stats[3] = (uint64_t)g.pw;
  d->pv_stats[4] = (uint64_t)g.ph;
  const bool timed = d->profiling != 0;
  if (timed) {
    for (hipEvent_t& e : d->ev_pv)
      if (!e) HIPCHK(hipEventCreateWithFlags(&e, kTimingEventFlags));
    HIPCHK(hipEventRecord(d->ev_pv[0], d->st));
  }
  HIPCHK(launch_preview(src, fmt, g.W, g.H, g.s, d->d_pv, d->st));
  std::vector<DrawPrim> prims;
  preview_prims(g, dets, n, boxes, nb, &prims);
  const int rc = draw_prims(d, prims, d->d_pv, g.pw, g.ph);
  if (rc != AT_OK) return rc;
  if (timed) HIPCHK(hipEventRecord(d->ev_pv[1], d->st));
  return AT_OK;
}

// after the stream was waited for: the time of k_preview and the drawing
static int preview_time(at_detector* d) {
  if (!d->profiling) return AT_OK;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, d->ev_pv[0], d->ev_pv[1]));
  d->pv_stats[5] += (uint64_t)((double)ms * 1e6);
  return AT_OK;
}

static bool preview_args_ok(const at_detector* d, const at_detection* dets, int n, const at_gp_box* boxes, int nb) {
  return d && n >= 0 && (n == 0 || dets) && nb >= 0 && (nb == 0 || boxes);
}

int at_preview_bgr(at_detector* d, int frame, int scale, const at_detection* dets, int n, const at_gp_box* boxes,
                   int nb, uint8_t* bgr_out) {
  PvGeom g;
  if (!preview_args_ok(d, dets, n, boxes, nb) || !bgr_out || !pv_geom(d->g.W, d->g.H, scale, &g)) return AT_E_INVALID;
  const uint8_t* src = nullptr;
  int fmt = 0;
  int rc = preview_source(d, frame, &src, &fmt);
  if (rc != AT_OK) return rc;
  rc = preview_draw(d, src, fmt, g, dets, n, boxes, nb);
  if (rc != AT_OK) return rc;
  const size_t bytes = (size_t)g.pw * g.ph * 3;
  HIPCHK(hipMemcpyAsync(bgr_out, d->d_pv, bytes, hipMemcpyDeviceToHost, d->st));
  HIPCHK(hipStreamSynchronize(d->st));
  d->pv_stats[0] = bytes;
  return preview_time(d);
}

// the encode (with the budget search) of the preview of `src`
static int preview_jpeg(at_detector* d, const uint8_t* src, int fmt, const PvGeom& g, const at_detection* dets, int n,
                        const at_gp_box* boxes, int nb, int quality, int sampling, size_t max_bytes, uint8_t* out,
                        size_t cap, size_t* len, int* quality_used) {
  int rc = preview_draw(d, src, fmt, g, dets, n, boxes, nb);
  if (rc != AT_OK) return rc;
  uint64_t enc_ns = 0;
  int qu = 0, encodes = 0;
  rc = preview_budget_search(
      quality, max_bytes, cap,
      [&](int q, size_t limit, size_t* l) {
        const int e = encode_jpeg(d, d->d_pv, q, sampling, out, limit, l, g.pw, g.ph);
        enc_ns += d->jpg_stats[1];
        return e;
      },
      len, &qu, &encodes);
  if (quality_used) *quality_used = qu;
  d->pv_stats[0] = *len;
  d->pv_stats[1] = (uint64_t)qu;
  d->pv_stats[2] = (uint64_t)encodes;
  if (rc != AT_OK && rc != AT_E_CAPACITY) return rc;
  const int trc = preview_time(d);  // (every encode waited for the stream)
  d->pv_stats[5] += enc_ns;
  return trc != AT_OK ? trc : rc;
}

static bool preview_jpeg_args_ok(const PvGeom& g, int quality, int sampling, const uint8_t* out, const size_t* len) {
  JpgGeom jg;
  return out && len && quality >= 1 && quality <= 100 && jpg_geom(g.pw, g.ph, sampling, &jg);
}

int at_preview_jpeg(at_detector* d, int frame, int scale, const at_detection* dets, int n, const at_gp_box* boxes,
                    int nb, int quality, int sampling, size_t max_bytes, uint8_t* out, size_t cap, size_t* len,
                    int* quality_used) {
  if (len) *len = 0;
  if (quality_used) *quality_used = 0;
  PvGeom g;
  if (!preview_args_ok(d, dets, n, boxes, nb) || !pv_geom(d->g.W, d->g.H, scale, &g) ||
      !preview_jpeg_args_ok(g, quality, sampling, out, len))
    return AT_E_INVALID;
  const uint8_t* src = nullptr;
  int fmt = 0;
  const int rc = preview_source(d, frame, &src, &fmt);
  if (rc != AT_OK) return rc;
  return preview_jpeg(d, src, fmt, g, dets, n, boxes, nb, quality, sampling, max_bytes, out, cap, len, quality_used);
}

int at_preview_jpeg_device(at_detector* d, const void* d_frame, at_pixfmt fmt, int scale, const at_detection* dets,
                           int n, const at_gp_box* boxes, int nb, int quality, int sampling, size_t max_bytes,
                           uint8_t* out, size_t cap, size_t* len, int* quality_used) {
  if (len) *len = 0;
  if (quality_used) *quality_used = 0;
  PvGeom g;
  if (!preview_args_ok(d, dets, n, boxes, nb) || !d_frame || ((uintptr_t)d_frame & 7) || !check_fmt(fmt) ||
      !pv_geom(d->g.W, d->g.H, scale, &g) || !preview_jpeg_args_ok(g, quality, sampling, out, len))
    return AT_E_INVALID;
  HIPCHK(hipSetDevice(d->device));
  return preview_jpeg(d, (const uint8_t*)d_frame, fmt, g, dets, n, boxes, nb, quality, sampling, max_bytes, out, cap,
                      len, quality_used);
}

int at_preview_stats(at_detector* d, uint64_t* out, int cap) {
  if (!d || !out || cap < 1) return AT_E_INVALID;
  const int n = std::min(cap, 6);
  for (int i = 0; i < n; i++) out[i] = d->pv_stats[i];
  return n;
}

int at_host_alloc(size_t bytes, void** out) {
  if (!out) return AT_E_INVALID;
  *out = nullptr;
  if (hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) {
    *out = nullptr;
    return AT_E_NOMEM;
  }
  return AT_OK;
}

void at_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

// ---- shared game-piece preprocessing ---------------------
static void drop_graphs(at_detector* d) {
  for (auto& kv : d->graphs) (void)hipGraphExecDestroy(kv.second);
  d->graphs.clear();
  for (auto& kv : d->split_graphs)
    for (auto* g : kv.second.seg) (void)hipGraphExecDestroy(g);
  d->split_graphs.clear();
}

int at_gp_enable(at_detector* d, int out_width, int out_height, int channels) {
  if (!d || out_width < 1 || out_height < 1 || out_width > 8192 || out_height > 8192 ||
      (channels != 1 && channels != 3))
    return AT_E_INVALID;
  if (hipSetDevice(d->device) != hipSuccess) return AT_E_HIP;
  if (d->pending && hipEventSynchronize(d->ev_done) != hipSuccess) return AT_E_HIP;
  const size_t bytes = (size_t)d->B * channels * out_width * out_height * sizeof(float);
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return AT_E_NOMEM;
  if (d->d.gp_out) {
    for (auto& a : d->allocs)
      if (a == d->d.gp_out) a = nullptr;
    (void)hipFree(d->d.gp_out);
  }
  d->allocs.push_back(p);
  d->d.gp_out = (float*)p;
  d->prm.gp_w = out_width;
  d->prm.gp_h = out_height;
  d->prm.gp_c = channels;
  d->last_gp = 0;  // no tensor until a BGR8 batch has produced one
  drop_graphs(d);  // the captured sequences carry the old parameters
  return AT_OK;
}

// ---- field pose --------------------------------------------------------------
// The layout lives in HBM (id table + tags, uploaded here, synchronously: no batch is
// pending); k_field joins the launch sequence behind k_pose while a layout is set, so the
// captured sequences are dropped whenever it changes.
int at_set_field_layout(at_detector* d, const at_field_tag* tags, int n, int max_hamming) {
  if (!d || max_hamming < 0 || !(d->prm.tag_size > 0) || d->pending) return AT_E_INVALID;
  std::vector<int16_t> lut(kFpMaxIds);
  std::vector<FpTag> lt;
  const int rc = fp_build_layout(tags, n, lut.data(), &lt);
  if (rc != AT_OK) return rc;
  if (hipSetDevice(d->device) != hipSuccess) return AT_E_HIP;
  if (n == 0) {
    if (d->field_on) drop_graphs(d);
    d->field_on = 0;
    return AT_OK;
  }
  FieldBufs& fb = d->field.b;
  if (!fb.out) {
    const size_t B = (size_t)d->B;
    void *plut = nullptr, *ptags = nullptr, *pout = nullptr;
    FpRecord* hrec = nullptr;
    void* hdev = nullptr;
    bool ok = hipMalloc(&plut, kFpMaxIds * sizeof(int16_t)) == hipSuccess &&
              hipMalloc(&ptags, kFpMaxIds * sizeof(FpTag)) == hipSuccess &&
              hipMalloc(&pout, B * sizeof(FpRecord)) == hipSuccess &&
              hipHostMalloc((void**)&hrec, B * sizeof(FpRecord), hipHostMallocMapped) == hipSuccess;
    int err = ok ? AT_OK : AT_E_NOMEM;
    if (ok && hipHostGetDevicePointer(&hdev, hrec, 0) != hipSuccess) err = AT_E_HIP;
    if (err == AT_OK) {
      for (int i = 0; i < 2 && err == AT_OK; i++)
        if (!d->ev_field[i] && hipEventCreateWithFlags(&d->ev_field[i], kTimingEventFlags) != hipSuccess) err = AT_E_HIP;
    }
    if (err != AT_OK) {
      if (plut) (void)hipFree(plut);
      if (ptags) (void)hipFree(ptags);
      if (pout) (void)hipFree(pout);
      if (hrec) (void)hipHostFree(hrec);
      return err;
    }
    d->allocs.push_back(plut);
    d->allocs.push_back(ptags);
    d->allocs.push_back(pout);
    memset(hrec, 0, B * sizeof(FpRecord));
    d->h_field = hrec;
    fb.lay.lut = (const int16_t*)plut;
    fb.lay.tags = (const FpTag*)ptags;
    fb.out = (FpRecord*)pout;
    fb.hout = (FpRecord*)hdev;
  }
  HIPCHK(hipMemcpy((void*)fb.lay.lut, lut.data(), kFpMaxIds * sizeof(int16_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((void*)fb.lay.tags, lt.data(), lt.size() * sizeof(FpTag), hipMemcpyHostToDevice));
  fb.lay.max_hamming = max_hamming;
  d->field_on = 1;
  drop_graphs(d);  // the captured sequences carry the old parameters
  return AT_OK;
}

int at_field_poses(at_detector* d, at_field_pose* out, int cap) {
  if (!d || cap < 0 || (cap > 0 && !out)) return AT_E_INVALID;
  if (d->pending) return AT_E_INVALID;  // collect first
  const int nf = d->last_nframes;
  for (int f = 0; f < nf && f < cap; f++) {
    if (d->last_field) fp_write(d->h_field[f], out + f);
    else memset(out + f, 0, sizeof(*out));
  }
  return nf;
}

int at_field_stats(at_detector* d, uint64_t* out, int cap) {
  if (!d || !out || cap < 1) return AT_E_INVALID;
  if (d->pending) return AT_E_INVALID;
  uint64_t v[5] = {0, 0, 0, 0, d->field_ns};
  if (d->last_field)
    for (int f = 0; f < d->last_nframes; f++) {
      const FpRecord& r = d->h_field[f];
      v[0] += r.n_tags > 0;
      v[1] += (uint64_t)r.n_tags;
      v[2] += (uint64_t)r.dropped;
      v[3] += (uint64_t)r.rejected;
    }
  const int n = std::min(cap, 5);
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}

// ---- ideal corners -------------------------------------------------------------
// The pose stage's head (k_pose, the pose wave of k_decode) maps every candidate's corners
// through und_point and writes an ideal record per slot beside the detection; the field and
// rig poses read those.  The side array and its mapped mirror are allocated at the first call;
// the kernels of a sequence are chosen by Params::undistort, so the captured sequences are
// dropped whenever it changes.
int at_set_undistort(at_detector* d, int on) {
  if (!d || d->pending || !(d->prm.tag_size > 0)) return AT_E_INVALID;
  on = on ? 1 : 0;
  if (hipSetDevice(d->device) != hipSuccess) return AT_E_HIP;
  if (on && !d->d.und) {
    const size_t B = (size_t)d->B;
    void* pund = nullptr;
    UndRecord* hrec = nullptr;
    void* hdev = nullptr;
    const bool ok = hipMalloc(&pund, B * kMaxDets * sizeof(UndRecord)) == hipSuccess &&
                    hipHostMalloc((void**)&hrec, B * kDetPoolPerFrame * sizeof(UndRecord), hipHostMallocMapped) == hipSuccess;
    int err = ok ? AT_OK : AT_E_NOMEM;
    if (ok && hipHostGetDevicePointer(&hdev, hrec, 0) != hipSuccess) err = AT_E_HIP;
    if (err != AT_OK) {
      if (pund) (void)hipFree(pund);
      if (hrec) (void)hipHostFree(hrec);
      return err;
    }
    d->allocs.push_back(pund);
    memset(hrec, 0, B * kDetPoolPerFrame * sizeof(UndRecord));
    d->h_und = hrec;
    d->d.und = (UndRecord*)pund;
    d->d.hund = (UndRecord*)hdev;
    d->und_ovf.resize(B);
  }
  if (d->prm.undistort != on) {
    d->prm.undistort = on;
    drop_graphs(d);  // the captured sequences carry the old kernels
  }
  return AT_OK;
}

// (the CPU twins at_ideal_detections_host and at_undistort_points_host: at_undist.cpp)

// the ideal record of result i of `frame` (the candidate's slot in the frame's pool)
static int und_record(at_detector* d, int frame, int k, const UndRecord** out) {
  const int ncand = (int)std::min<uint32_t>(d->h_ctrl[kCtlNdets * d->B + frame], kMaxDets);
  if (ncand <= kDetPoolPerFrame) {
    *out = d->h_und + (size_t)frame * kDetPoolPerFrame + k;
    return AT_OK;
  }
  std::vector<UndRecord>& v = d->und_ovf[frame];
  if ((int)v.size() != ncand) {  // (cleared at every enqueue)
    v.resize(ncand);
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipMemcpyAsync(v.data(), d->d.und + (size_t)frame * kMaxDets, ncand * sizeof(UndRecord), hipMemcpyDeviceToHost,
                          d->st));
    HIPCHK(hipStreamSynchronize(d->st));
  }
  *out = v.data() + k;
  return AT_OK;
}

int at_ideal_detections(at_detector* d, int frame, at_detection* out, int cap) {
  if (!d || frame < 0 || frame >= d->last_nframes || (cap > 0 && !out)) return AT_E_INVALID;
  if (d->pending || !d->last_und) return AT_E_INVALID;
  const int n = d->res_n[frame];
  for (int i = 0; i < n && i < cap; i++) {
    const int k = d->res_idx[(size_t)frame * kMaxDets + i];
    write_detection(d->res_base[frame][k], out + i);
    const UndRecord* u = nullptr;
    const int rc = und_record(d, frame, k, &u);
    if (rc != AT_OK) return rc;
    out[i].id = u->id;
    memcpy(out[i].H, u->H, sizeof(u->H));
    memcpy(out[i].c, u->c, sizeof(u->c));
    memcpy(out[i].p, u->p, sizeof(u->p));
  }
  return n;
}

int at_undistort_points(at_detector* d, const double* xy, int n, double* out_xy, uint8_t* ok) {
  if (!d || n < 0 || n > (1 << 24) || (n > 0 && (!xy || !out_xy || !ok))) return AT_E_INVALID;
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(d->device));
  if ((size_t)n > d->undpts_cap) {
    size_t cap = std::max<size_t>(1024, d->undpts_cap);
    while (cap < (size_t)n) cap *= 2;
    void* p = nullptr;
    if (hipMalloc(&p, cap * 40) != hipSuccess) return AT_E_NOMEM;  // 16 B in, 16 B out, a flag (in 8)
    HIPCHK(hipStreamSynchronize(d->st));
    if (d->d_undpts) (void)hipFree(d->d_undpts);
    d->d_undpts = p;
    d->undpts_cap = cap;
  }
  double* din = (double*)d->d_undpts;
  double* dout = din + 2 * d->undpts_cap;
  uint8_t* dok = (uint8_t*)(dout + 2 * d->undpts_cap);
  const UndCam c = {d->prm.fx, d->prm.fy, d->prm.cx, d->prm.cy, d->prm.k1, d->prm.k2, d->prm.p1, d->prm.p2, d->prm.k3};
  HIPCHK(hipMemcpyAsync(din, xy, (size_t)n * 16, hipMemcpyHostToDevice, d->st));
  HIPCHK(launch_und_points(c, din, n, dout, dok, d->st));
  HIPCHK(hipMemcpyAsync(out_xy, dout, (size_t)n * 16, hipMemcpyDeviceToHost, d->st));
  HIPCHK(hipMemcpyAsync(ok, dok, (size_t)n, hipMemcpyDeviceToHost, d->st));
  HIPCHK(hipStreamSynchronize(d->st));
  return n;
}

int at_undistort_stats(at_detector* d, uint64_t* out, int cap) {
  if (!d || !out || cap < 1) return AT_E_INVALID;
  if (d->pending) return AT_E_INVALID;
  uint64_t v[2] = {0, 0};
  if (d->last_und)
    for (int f = 0; f < d->last_nframes; f++)
      for (int i = 0; i < d->res_n[f]; i++) {
        const UndRecord* u = nullptr;
        const int rc = und_record(d, f, d->res_idx[(size_t)f * kMaxDets + i], &u);
        if (rc != AT_OK) return rc;
        v[u->id < 0 ? 1 : 0]++;
      }
  const int n = std::min(cap, 2);
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}

// ---- rig pose ------------------------------------------------------------------
// The rig owns its stream, its copy of the layout in HBM and one record per instant in HBM and
// in mapped host memory; of its members it holds pointers only (their candidates, counts and
// completion events), and k_rig reads them.
struct at_rig {
  int n_cams;
  int device;
  int B;                     // most instants: the smallest max_batch of the members
  at_detector* det[kRigMaxCams];
  hipStream_t st;
  hipEvent_t ev[2];          // around k_rig while a member profiles
  RigBufs b;
  void *d_lut, *d_tags, *d_out;
  RigRecord* h_out;          // [B] the host side of b.hout
  int last_n;                // instants of the last solve
  uint64_t ns;               // k_rig's time of the last solve (while profiling)
  // the robust solve's own records and infos, allocated at the first at_rig_solve_robust: what
  // at_rig_solve and at_rig_stats read above is never written by it
  void *xd_out, *xd_info;
  RigRecord* xh_out;         // [B]
  RigRobustInfo* xh_info;    // [B]
  RigRobustBufs xb;
  int xlast_n;               // instants of the last robust solve
  uint64_t xns;              // k_rig_robust's time of the last robust solve (while profiling)
};

void at_rig_destroy(at_rig* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->st) (void)hipStreamSynchronize(r->st);
  if (r->d_lut) (void)hipFree(r->d_lut);
  if (r->d_tags) (void)hipFree(r->d_tags);
  if (r->d_out) (void)hipFree(r->d_out);
  if (r->h_out) (void)hipHostFree(r->h_out);
  if (r->xd_out) (void)hipFree(r->xd_out);
  if (r->xd_info) (void)hipFree(r->xd_info);
  if (r->xh_out) (void)hipHostFree(r->xh_out);
  if (r->xh_info) (void)hipHostFree(r->xh_info);
  for (hipEvent_t e : r->ev)
    if (e) (void)hipEventDestroy(e);
  if (r->st) (void)hipStreamDestroy(r->st);
  delete r;
}

int at_rig_create(at_detector* const* dets, const at_rig_extrinsics* extr, int n_cams, const at_field_tag* tags,
                  int n_tags, int max_hamming, at_rig** out) {
  if (!out || !dets || !extr || n_cams < 1 || n_cams > kRigMaxCams || max_hamming < 0 || n_tags < 1)
    return AT_E_INVALID;
  int B = 0;
  for (int i = 0; i < n_cams; i++) {
    const at_detector* d = dets[i];
    if (!d || !(d->prm.tag_size > 0) || d->device != dets[0]->device || d->prm.tag_size != dets[0]->prm.tag_size)
      return AT_E_INVALID;
    for (int k = 0; k < i; k++)
      if (dets[k] == d) return AT_E_INVALID;
    if (!rig_extrinsics_ok(extr[i])) return AT_E_INVALID;
    B = i ? std::min(B, d->B) : d->B;
  }
  std::vector<int16_t> lut(kFpMaxIds);
  std::vector<FpTag> lt;
  const int rc = fp_build_layout(tags, n_tags, lut.data(), &lt);
  if (rc != AT_OK) return rc;
  if (hipSetDevice(dets[0]->device) != hipSuccess) return AT_E_HIP;
  at_rig* r = new at_rig();
  r->n_cams = n_cams;
  r->device = dets[0]->device;
  r->B = B;
  void* hdev = nullptr;
  int err = AT_OK;
  if (hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking) != hipSuccess) err = AT_E_HIP;
  for (int i = 0; i < 2 && err == AT_OK; i++)
    if (hipEventCreateWithFlags(&r->ev[i], kTimingEventFlags) != hipSuccess) err = AT_E_HIP;
  if (err == AT_OK && !(hipMalloc(&r->d_lut, kFpMaxIds * sizeof(int16_t)) == hipSuccess &&
                        hipMalloc(&r->d_tags, lt.size() * sizeof(FpTag)) == hipSuccess &&
                        hipMalloc(&r->d_out, (size_t)B * sizeof(RigRecord)) == hipSuccess &&
                        hipHostMalloc((void**)&r->h_out, (size_t)B * sizeof(RigRecord), hipHostMallocMapped) ==
                            hipSuccess))
    err = AT_E_NOMEM;
  if (err == AT_OK && hipHostGetDevicePointer(&hdev, r->h_out, 0) != hipSuccess) err = AT_E_HIP;
  if (err == AT_OK && !(hipMemcpy(r->d_lut, lut.data(), kFpMaxIds * sizeof(int16_t), hipMemcpyHostToDevice) ==
                            hipSuccess &&
                        hipMemcpy(r->d_tags, lt.data(), lt.size() * sizeof(FpTag), hipMemcpyHostToDevice) ==
                            hipSuccess))
    err = AT_E_HIP;
  if (err != AT_OK) {
    at_rig_destroy(r);
    return err;
  }
  memset(r->h_out, 0, (size_t)B * sizeof(RigRecord));
  RigBufs& b = r->b;
  for (int i = 0; i < n_cams; i++) {
    at_detector* d = dets[i];
    r->det[i] = d;
    RigCamView& v = b.view[i];
    v.dets = d->d.dets;
    v.ndets = d->d.ndets;
    v.cam = {d->prm.fx, d->prm.fy, d->prm.cx, d->prm.cy, {}, {}};
    v.und = nullptr;  // (at_rig_solve sets it)
    memcpy(v.cam.ER, extr[i].R, sizeof(v.cam.ER));
    memcpy(v.cam.Et, extr[i].t, sizeof(v.cam.Et));
  }
  b.lay.lut = (const int16_t*)r->d_lut;
  b.lay.tags = (const FpTag*)r->d_tags;
  b.lay.max_hamming = max_hamming;
  b.out = (RigRecord*)r->d_out;
  b.hout = (RigRecord*)hdev;
  b.tag_size = dets[0]->prm.tag_size;
  b.n_cams = n_cams;
  *out = r;
  return AT_OK;
}

int at_rig_solve(at_rig* r, at_rig_pose* out, int cap) {
  if (!r || cap < 0 || (cap > 0 && !out)) return AT_E_INVALID;
  const int n = r->det[0]->last_nframes;
  if (n < 1 || n > r->B) return AT_E_INVALID;
  bool timed = false;
  for (int i = 0; i < r->n_cams; i++) {
    if (r->det[i]->last_nframes != n) return AT_E_INVALID;
    timed = timed || r->det[i]->profiling;
  }
  if (hipSetDevice(r->device) != hipSuccess) return AT_E_HIP;
  // behind every member's batch (an event of a batch already collected is complete)
  for (int i = 0; i < r->n_cams; i++) HIPCHK(hipStreamWaitEvent(r->st, r->det[i]->ev_done, 0));
  // a member whose last batch ran with at_set_undistort on is read through its ideal records
  for (int i = 0; i < r->n_cams; i++) r->b.view[i].und = r->det[i]->last_und ? r->det[i]->d.und : nullptr;
  if (timed) HIPCHK(hipEventRecord(r->ev[0], r->st));
  HIPCHK(launch_rig(r->b, n, r->st));
  if (timed) HIPCHK(hipEventRecord(r->ev[1], r->st));
  HIPCHK(hipStreamSynchronize(r->st));
  r->ns = 0;
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, r->ev[0], r->ev[1]));
    r->ns = (uint64_t)((double)ms * 1e6);
  }
  r->last_n = n;
  for (int f = 0; f < n && f < cap; f++) rig_write(r->h_out[f], out + f);
  return n;
}

int at_rig_stats(at_rig* r, uint64_t* out, int cap) {
  if (!r || !out || cap < 1) return AT_E_INVALID;
  uint64_t v[5] = {0, 0, 0, 0, r->ns};
  for (int f = 0; f < r->last_n; f++) {
    const RigRecord& q = r->h_out[f];
    v[0] += q.n_tags > 0;
    v[1] += (uint64_t)q.n_tags;
    v[2] += (uint64_t)q.dropped;
    v[3] += (uint64_t)q.rejected;
  }
  const int n = std::min(cap, 5);
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}

// ---- robust rig pose -------------------------------------------------------------
static int rig_robust_reserve(at_rig* r) {
  if (r->xh_info) return AT_OK;
  const size_t B = (size_t)r->B;
  void *ho = nullptr, *hi = nullptr;
  int err = AT_OK;
  if (!(hipMalloc(&r->xd_out, B * sizeof(RigRecord)) == hipSuccess &&
        hipMalloc(&r->xd_info, B * sizeof(RigRobustInfo)) == hipSuccess &&
        hipHostMalloc((void**)&r->xh_out, B * sizeof(RigRecord), hipHostMallocMapped) == hipSuccess &&
        hipHostMalloc((void**)&r->xh_info, B * sizeof(RigRobustInfo), hipHostMallocMapped) == hipSuccess))
    err = AT_E_NOMEM;
  if (err == AT_OK && !(hipHostGetDevicePointer(&ho, r->xh_out, 0) == hipSuccess &&
                        hipHostGetDevicePointer(&hi, r->xh_info, 0) == hipSuccess))
    err = AT_E_HIP;
  if (err != AT_OK) {  // all or nothing: a later call starts over
    if (r->xd_out) (void)hipFree(r->xd_out);
    if (r->xd_info) (void)hipFree(r->xd_info);
    if (r->xh_out) (void)hipHostFree(r->xh_out);
    if (r->xh_info) (void)hipHostFree(r->xh_info);
    r->xd_out = r->xd_info = nullptr;
    r->xh_out = nullptr;
    r->xh_info = nullptr;
    return err;
  }
  memset(r->xh_out, 0, B * sizeof(RigRecord));
  memset(r->xh_info, 0, B * sizeof(RigRobustInfo));
  r->xb.out = (RigRecord*)r->xd_out;
  r->xb.hout = (RigRecord*)ho;
  r->xb.info = (RigRobustInfo*)r->xd_info;
  r->xb.hinfo = (RigRobustInfo*)hi;
  return AT_OK;
}

int at_rig_solve_robust(at_rig* r, const at_rig_robust_config* cfg, at_rig_pose* out, at_rig_robust_info* info,
                        int cap) {
  if (!r || cap < 0 || (cap > 0 && (!out || !info))) return AT_E_INVALID;
  RigRobustCfg c;
  if (!rig_robust_config(cfg, &c)) return AT_E_INVALID;
  const int n = r->det[0]->last_nframes;
  if (n < 1 || n > r->B) return AT_E_INVALID;
  bool timed = false;
  for (int i = 0; i < r->n_cams; i++) {
    if (r->det[i]->last_nframes != n) return AT_E_INVALID;
    timed = timed || r->det[i]->profiling;
  }
  if (hipSetDevice(r->device) != hipSuccess) return AT_E_HIP;
  const int rc = rig_robust_reserve(r);
  if (rc != AT_OK) return rc;
  r->xb.cfg = c;
  // behind every member's batch, through the members' ideal records where they have them: at_rig_solve's
  for (int i = 0; i < r->n_cams; i++) HIPCHK(hipStreamWaitEvent(r->st, r->det[i]->ev_done, 0));
  for (int i = 0; i < r->n_cams; i++) r->b.view[i].und = r->det[i]->last_und ? r->det[i]->d.und : nullptr;
  if (timed) HIPCHK(hipEventRecord(r->ev[0], r->st));
  HIPCHK(launch_rig_robust(r->b, r->xb, n, r->st));
  if (timed) HIPCHK(hipEventRecord(r->ev[1], r->st));
  HIPCHK(hipStreamSynchronize(r->st));
  r->xns = 0;
  if (timed) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, r->ev[0], r->ev[1]));
    r->xns = (uint64_t)((double)ms * 1e6);
  }
  r->xlast_n = n;
  for (int f = 0; f < n && f < cap; f++) {
    rig_write(r->xh_out[f], out + f);
    memcpy(info + f, &r->xh_info[f], sizeof(*info));
  }
  return n;
}

int at_rig_robust_stats(at_rig* r, uint64_t* out, int cap) {
  if (!r || !out || cap < 1) return AT_E_INVALID;
  uint64_t v[5] = {0, 0, 0, 0, r->xns};
  for (int f = 0; f < r->xlast_n; f++) {
    const RigRobustInfo& q = r->xh_info[f];
    v[0] += r->xh_out[f].n_tags > 0;
    v[1] += (uint64_t)q.n_rejected;
    v[2] += (uint64_t)q.rounds;
    v[3] += (uint64_t)q.starved;
  }
  const int n = std::min(cap, 5);
  for (int i = 0; i < n; i++) out[i] = v[i];
  return n;
}

// ---- rig calibration -----------------------------------------------------------
// The device side of an at_rigcal (at_rigcal.cpp holds the rest): a stream and two events of its
// own, the layout and the stored instants in HBM, the solve's buffers sized for the instants
// stored so far (grown by doubling), and pinned host memory for what comes back.
namespace at {
struct CalGpu {
  int device;
  hipStream_t st;
  hipEvent_t ev[2];
  int cap_n;  // instants the buffers hold
  std::vector<void*> dev, host;
  CalBufs b;  // device pointers
  CalPose *h_pose[2], *h_ext[2];
  double *h_instcost, *h_cov;
  int32_t* h_ntags;
  CalCtl* h_ctl;
};
}  // namespace at

static void calgpu_release(CalGpu* g) {
  for (void* p : g->dev) (void)hipFree(p);
  for (void* p : g->host) (void)hipHostFree(p);
  g->dev.clear();
  g->host.clear();
  g->cap_n = 0;
}

static void calgpu_free(CalGpu* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->st) (void)hipStreamSynchronize(g->st);
  calgpu_release(g);
  for (hipEvent_t e : g->ev)
    if (e) (void)hipEventDestroy(e);
  if (g->st) (void)hipStreamDestroy(g->st);
  delete g;
}

static int calgpu_reserve(at_rigcal* c, CalGpu* g, int n) {
  if (hipStreamSynchronize(g->st) != hipSuccess) return AT_E_HIP;
  calgpu_release(g);
  bool ok = true;
  auto dmal = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (!ok || hipMalloc(&p, bytes) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    g->dev.push_back(p);
    return p;
  };
  auto hmal = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (!ok || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    g->host.push_back(p);
    return p;
  };
  CalBufs& b = g->b;
  memset(&b, 0, sizeof(b));
  b.n_cams = c->n_cams;
  b.N = n;
  const size_t N = (size_t)n, nc = (size_t)c->n_cams, E = (size_t)b.E();
  b.obs = (const CalCamObs*)dmal(N * nc * sizeof(CalCamObs));
  b.rec = (RigRecord*)dmal(N * sizeof(RigRecord));
  b.ntags = (int32_t*)dmal(N * sizeof(int32_t));
  for (int q = 0; q < 2; q++) {
    b.pose[q] = (CalPose*)dmal(N * sizeof(CalPose));
    b.ext[q] = (CalPose*)dmal(nc * sizeof(CalPose));
    g->h_pose[q] = (CalPose*)hmal(N * sizeof(CalPose));
    g->h_ext[q] = (CalPose*)hmal(nc * sizeof(CalPose));
  }
  b.inst = (double*)dmal(N * (size_t)b.inst_len() * sizeof(double));
  b.part = (double*)dmal(N * E * sizeof(double));
  b.chunk = (double*)dmal((size_t)b.chunks() * E * sizeof(double));
  b.dc = (double*)dmal((size_t)b.M() * sizeof(double));
  b.instcost = (double*)dmal(N * sizeof(double));
  b.cov = (double*)dmal(nc * 36 * sizeof(double));
  b.ctl = (CalCtl*)dmal(sizeof(CalCtl));
  b.lay.lut = (const int16_t*)dmal(kFpMaxIds * sizeof(int16_t));
  b.lay.tags = (const FpTag*)dmal(c->tags.size() * sizeof(FpTag));
  b.lay.max_hamming = c->max_hamming;
  g->h_instcost = (double*)hmal(N * sizeof(double));
  g->h_cov = (double*)hmal(nc * 36 * sizeof(double));
  g->h_ntags = (int32_t*)hmal(N * sizeof(int32_t));
  g->h_ctl = (CalCtl*)hmal(sizeof(CalCtl));
  if (!ok) {
    calgpu_release(g);
    return AT_E_NOMEM;
  }
  if (hipMemcpy((void*)b.lay.lut, c->lut.data(), kFpMaxIds * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy((void*)b.lay.tags, c->tags.data(), c->tags.size() * sizeof(FpTag), hipMemcpyHostToDevice) !=
          hipSuccess) {
    calgpu_release(g);
    return AT_E_HIP;
  }
  g->cap_n = n;
  c->obs_dirty = true;
  return AT_OK;
}

int at_rigcal_solve(at_rigcal* c, at_rigcal_result* out) {
  if (!c || !out || c->n < 1) return AT_E_INVALID;
  CalGpu* g = c->gpu;
  if (!g) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AT_E_HIP;
    g = new CalGpu();
    g->device = dev;
    bool ok = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++) ok = hipEventCreateWithFlags(&g->ev[i], kTimingEventFlags) == hipSuccess;
    if (!ok) {
      calgpu_free(g);
      return AT_E_HIP;
    }
    c->gpu = g;
    c->gpu_free = calgpu_free;
  }
  if (hipSetDevice(g->device) != hipSuccess) return AT_E_HIP;
  if (c->n > g->cap_n) {
    const int rc = calgpu_reserve(c, g, std::min(kCalMaxInstants, std::max(c->n, 2 * g->cap_n)));
    if (rc != AT_OK) return rc;
  }
  // (the buffers may hold more instants than are stored: the strides depend on n_cams only)
  CalBufs b = g->b;
  const FpLayout lay = b.lay;
  cal_fill_bufs(*c, &b);
  b.lay = lay;
  const size_t N = (size_t)c->n, nc = (size_t)c->n_cams;
  if (c->obs_dirty) {
    HIPCHK(hipMemcpyAsync((void*)b.obs, c->obs.data(), N * nc * sizeof(CalCamObs), hipMemcpyHostToDevice, g->st));
    c->obs_dirty = false;
  }
  for (size_t i = 0; i < nc; i++) {
    memcpy(g->h_ext[0][i].R, c->cams[i].extr.R, sizeof(g->h_ext[0][i].R));
    memcpy(g->h_ext[0][i].t, c->cams[i].extr.t, sizeof(g->h_ext[0][i].t));
  }
  for (int q = 0; q < 2; q++)
    HIPCHK(hipMemcpyAsync(b.ext[q], g->h_ext[0], nc * sizeof(CalPose), hipMemcpyHostToDevice, g->st));
  HIPCHK(hipMemsetAsync(b.ctl, 0, sizeof(CalCtl), g->st));
  if (c->profiling) HIPCHK(hipEventRecord(g->ev[0], g->st));
  HIPCHK(launch_rigcal(b, g->st));
  if (c->profiling) HIPCHK(hipEventRecord(g->ev[1], g->st));
  // (h_ext[0] is read by the copies above, which the kernels and so these copies follow in order)
  HIPCHK(hipMemcpyAsync(g->h_ctl, b.ctl, sizeof(CalCtl), hipMemcpyDeviceToHost, g->st));
  for (int q = 0; q < 2; q++) {
    HIPCHK(hipMemcpyAsync(g->h_ext[q], b.ext[q], nc * sizeof(CalPose), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpyAsync(g->h_pose[q], b.pose[q], N * sizeof(CalPose), hipMemcpyDeviceToHost, g->st));
  }
  HIPCHK(hipMemcpyAsync(g->h_cov, b.cov, nc * 36 * sizeof(double), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(g->h_instcost, b.instcost, N * sizeof(double), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(g->h_ntags, b.ntags, N * sizeof(int32_t), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  uint64_t ns = 0;
  if (c->profiling) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]));
    ns = (uint64_t)((double)ms * 1e6);
  }
  const int w = g->h_ctl->which & 1;
  cal_finish(c, *g->h_ctl, g->h_ext[w], g->h_cov, g->h_pose[w], g->h_instcost, g->h_ntags, out);
  c->ns = ns;
  return AT_OK;
}

// ---- camera calibration --------------------------------------------------------
// The device side of an at_camcal (at_camcal.cpp holds the rest), as CalGpu: a stream and two
// events of its own, the board and the stored views in HBM, the solve's buffers sized for the
// views stored so far (grown by doubling), and pinned host memory for what comes back.
namespace at {
struct CcGpu {
  int device;
  hipStream_t st;
  hipEvent_t ev[2];
  int cap_n;  // views the buffers hold
  std::vector<void*> dev, host;
  CcBufs b;  // device pointers
  CalPose* h_pose[2];
  CcCam* h_cam;  // [2]
  double *h_viewcost, *h_cov;
  int32_t* h_ntags;
  CalCtl* h_ctl;
};
}  // namespace at

static void ccgpu_release(CcGpu* g) {
  for (void* p : g->dev) (void)hipFree(p);
  for (void* p : g->host) (void)hipHostFree(p);
  g->dev.clear();
  g->host.clear();
  g->cap_n = 0;
}

static void ccgpu_free(CcGpu* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->st) (void)hipStreamSynchronize(g->st);
  ccgpu_release(g);
  for (hipEvent_t e : g->ev)
    if (e) (void)hipEventDestroy(e);
  if (g->st) (void)hipStreamDestroy(g->st);
  delete g;
}

static int ccgpu_reserve(at_camcal* c, CcGpu* g, int n) {
  if (hipStreamSynchronize(g->st) != hipSuccess) return AT_E_HIP;
  ccgpu_release(g);
  bool ok = true;
  auto dmal = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (!ok || hipMalloc(&p, bytes) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    g->dev.push_back(p);
    return p;
  };
  auto hmal = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (!ok || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    g->host.push_back(p);
    return p;
  };
  CcBufs& b = g->b;
  memset(&b, 0, sizeof(b));
  b.N = n;
  const size_t N = (size_t)n;
  b.obs = (const CcObs*)dmal(N * sizeof(CcObs));
  b.ntags = (int32_t*)dmal(N * sizeof(int32_t));
  for (int q = 0; q < 2; q++) {
    b.pose[q] = (CalPose*)dmal(N * sizeof(CalPose));
    b.cam[q] = (CcCam*)dmal(sizeof(CcCam));
    g->h_pose[q] = (CalPose*)hmal(N * sizeof(CalPose));
  }
  b.view = (double*)dmal(N * kCcViewLen * sizeof(double));
  b.part = (double*)dmal(N * kCcE * sizeof(double));
  b.chunk = (double*)dmal((size_t)b.chunks() * kCcE * sizeof(double));
  b.dc = (double*)dmal(kCcP * sizeof(double));
  b.viewcost = (double*)dmal(N * sizeof(double));
  b.cov = (double*)dmal(81 * sizeof(double));
  b.ctl = (CalCtl*)dmal(sizeof(CalCtl));
  b.lay.lut = (const int16_t*)dmal(kFpMaxIds * sizeof(int16_t));
  b.lay.tags = (const FpTag*)dmal(c->tags.size() * sizeof(FpTag));
  b.lay.max_hamming = c->max_hamming;
  g->h_cam = (CcCam*)hmal(2 * sizeof(CcCam));
  g->h_viewcost = (double*)hmal(N * sizeof(double));
  g->h_cov = (double*)hmal(81 * sizeof(double));
  g->h_ntags = (int32_t*)hmal(N * sizeof(int32_t));
  g->h_ctl = (CalCtl*)hmal(sizeof(CalCtl));
  if (!ok) {
    ccgpu_release(g);
    return AT_E_NOMEM;
  }
  if (hipMemcpy((void*)b.lay.lut, c->lut.data(), kFpMaxIds * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy((void*)b.lay.tags, c->tags.data(), c->tags.size() * sizeof(FpTag), hipMemcpyHostToDevice) !=
          hipSuccess) {
    ccgpu_release(g);
    return AT_E_HIP;
  }
  g->cap_n = n;
  c->obs_dirty = true;
  return AT_OK;
}

int at_camcal_solve(at_camcal* c, at_camcal_result* out) {
  if (!c || !out || c->n < 1) return AT_E_INVALID;
  CcCam start;
  const int src = cc_start_camera(*c, &start);
  if (src != AT_OK) return src;
  CcGpu* g = c->gpu;
  if (!g) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AT_E_HIP;
    g = new CcGpu();
    g->device = dev;
    bool ok = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++) ok = hipEventCreateWithFlags(&g->ev[i], kTimingEventFlags) == hipSuccess;
    if (!ok) {
      ccgpu_free(g);
      return AT_E_HIP;
    }
    c->gpu = g;
    c->gpu_free = ccgpu_free;
  }
  if (hipSetDevice(g->device) != hipSuccess) return AT_E_HIP;
  if (c->n > g->cap_n) {
    const int rc = ccgpu_reserve(c, g, std::min(kCcMaxViews, std::max(c->n, 2 * g->cap_n)));
    if (rc != AT_OK) return rc;
  }
  // (the buffers may hold more views than are stored: no stride depends on the count)
  CcBufs b = g->b;
  b.N = c->n;
  b.tag_size = c->tag_size;
  b.free_mask = c->cfg.free_mask;
  const size_t N = (size_t)c->n;
  if (c->obs_dirty) {
    HIPCHK(hipMemcpyAsync((void*)b.obs, c->obs.data(), N * sizeof(CcObs), hipMemcpyHostToDevice, g->st));
    c->obs_dirty = false;
  }
  g->h_cam[0] = start;
  for (int q = 0; q < 2; q++)
    HIPCHK(hipMemcpyAsync(b.cam[q], &g->h_cam[0], sizeof(CcCam), hipMemcpyHostToDevice, g->st));
  HIPCHK(hipMemsetAsync(b.ctl, 0, sizeof(CalCtl), g->st));
  if (c->profiling) HIPCHK(hipEventRecord(g->ev[0], g->st));
  HIPCHK(launch_camcal(b, g->st));
  if (c->profiling) HIPCHK(hipEventRecord(g->ev[1], g->st));
  // (h_cam[0] is read by the copies above, which the kernels and so these copies follow in order)
  HIPCHK(hipMemcpyAsync(g->h_ctl, b.ctl, sizeof(CalCtl), hipMemcpyDeviceToHost, g->st));
  for (int q = 0; q < 2; q++) {
    HIPCHK(hipMemcpyAsync(&g->h_cam[q], b.cam[q], sizeof(CcCam), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpyAsync(g->h_pose[q], b.pose[q], N * sizeof(CalPose), hipMemcpyDeviceToHost, g->st));
  }
  HIPCHK(hipMemcpyAsync(g->h_cov, b.cov, 81 * sizeof(double), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(g->h_viewcost, b.viewcost, N * sizeof(double), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(g->h_ntags, b.ntags, N * sizeof(int32_t), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  uint64_t ns = 0;
  if (c->profiling) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]));
    ns = (uint64_t)((double)ms * 1e6);
  }
  const int w = g->h_ctl->which & 1;
  cc_finish(c, *g->h_ctl, g->h_cam[w], g->h_cov, g->h_pose[w], g->h_viewcost, g->h_ntags, out);
  c->ns = ns;
  return AT_OK;
}

// ---- field map -----------------------------------------------------------------
// The device side of an at_fieldmap (at_fieldmap.cpp holds the rest), as CalGpu: a stream and two
// events of its own, the stored views in HBM, the solve's buffers sized for the views stored so
// far (grown by doubling; those of the reduced system depend on the map's tag count only), and
// pinned host memory for what goes up and comes back.
namespace at {
struct FmGpu {
  int device;
  hipStream_t st;
  hipEvent_t ev[2];
  int cap_n;  // views the buffers hold
  std::vector<void*> dev, host;
  FmBufs b;  // device pointers
  CalPose *h_pose[2], *h_tag[2], *h_start;
  int16_t* h_lut;
  FpTag* h_lay;
  double *h_viewcost, *h_cov;
  int32_t* h_ntags;
  CalCtl* h_ctl;
};
}  // namespace at

static void fmgpu_release(FmGpu* g) {
  for (void* p : g->dev) (void)hipFree(p);
  for (void* p : g->host) (void)hipHostFree(p);
  g->dev.clear();
  g->host.clear();
  g->cap_n = 0;
}

static void fmgpu_free(FmGpu* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->st) (void)hipStreamSynchronize(g->st);
  fmgpu_release(g);
  for (hipEvent_t e : g->ev)
    if (e) (void)hipEventDestroy(e);
  if (g->st) (void)hipStreamDestroy(g->st);
  delete g;
}

static int fmgpu_reserve(at_fieldmap* m, FmGpu* g, int n) {
  if (hipStreamSynchronize(g->st) != hipSuccess) return AT_E_HIP;
  fmgpu_release(g);
  bool ok = true;
  auto dmal = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (!ok || hipMalloc(&p, bytes) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    g->dev.push_back(p);
    return p;
  };
  auto hmal = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (!ok || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    g->host.push_back(p);
    return p;
  };
  FmBufs& b = g->b;
  memset(&b, 0, sizeof(b));
  b.T = m->n_tags;
  b.N = n;
  const size_t N = (size_t)n, T = (size_t)m->n_tags, E = (size_t)b.E(), M = (size_t)b.M();
  b.obs = (const FmObs*)dmal(N * sizeof(FmObs));
  b.rec = (FpRecord*)dmal(N * sizeof(FpRecord));
  b.ntags = (int32_t*)dmal(N * sizeof(int32_t));
  for (int q = 0; q < 2; q++) {
    b.pose[q] = (CalPose*)dmal(N * sizeof(CalPose));
    b.tag[q] = (CalPose*)dmal(T * sizeof(CalPose));
    g->h_pose[q] = (CalPose*)hmal(N * sizeof(CalPose));
    g->h_tag[q] = (CalPose*)hmal(T * sizeof(CalPose));
  }
  b.view = (double*)dmal(N * kFmViewLen * sizeof(double));
  b.tab = (int32_t*)dmal(N * kFpMaxTags * sizeof(int32_t));
  b.inv = (int32_t*)dmal(N * kFmMaxTags * sizeof(int32_t));
  b.chunk = (double*)dmal((size_t)b.chunks() * E * sizeof(double));
  b.S = (double*)dmal(E * sizeof(double));
  b.A = (double*)dmal(M * M * sizeof(double));
  b.dc = (double*)dmal(M * sizeof(double));
  b.viewcost = (double*)dmal(N * sizeof(double));
  b.cov = (double*)dmal(T * 36 * sizeof(double));
  b.ctl = (CalCtl*)dmal(sizeof(CalCtl));
  b.lay.lut = (const int16_t*)dmal(kFpMaxIds * sizeof(int16_t));
  b.lay.tags = (const FpTag*)dmal(T * sizeof(FpTag));
  b.lay.max_hamming = m->max_hamming;
  g->h_start = (CalPose*)hmal(T * sizeof(CalPose));
  g->h_lut = (int16_t*)hmal(kFpMaxIds * sizeof(int16_t));
  g->h_lay = (FpTag*)hmal(T * sizeof(FpTag));
  g->h_viewcost = (double*)hmal(N * sizeof(double));
  g->h_cov = (double*)hmal(T * 36 * sizeof(double));
  g->h_ntags = (int32_t*)hmal(N * sizeof(int32_t));
  g->h_ctl = (CalCtl*)hmal(sizeof(CalCtl));
  if (!ok) {
    fmgpu_release(g);
    return AT_E_NOMEM;
  }
  g->cap_n = n;
  m->obs_dirty = true;
  return AT_OK;
}

int at_fieldmap_solve(at_fieldmap* m, at_fieldmap_result* out) {
  if (!m || !out || m->n < 1) return AT_E_INVALID;
  FmGpu* g = m->gpu;
  if (!g) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AT_E_HIP;
    g = new FmGpu();
    g->device = dev;
    bool ok = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++) ok = hipEventCreateWithFlags(&g->ev[i], kTimingEventFlags) == hipSuccess;
    if (!ok) {
      fmgpu_free(g);
      return AT_E_HIP;
    }
    m->gpu = g;
    m->gpu_free = fmgpu_free;
  }
  if (hipSetDevice(g->device) != hipSuccess) return AT_E_HIP;
  if (m->n > g->cap_n) {
    const int rc = fmgpu_reserve(m, g, std::min(kFmMaxViews, std::max(m->n, 2 * g->cap_n)));
    if (rc != AT_OK) return rc;
  }
  // (the buffers may hold more views than are stored: no stride depends on the count)
  FmBufs b = g->b;
  const FpLayout lay = b.lay;
  std::vector<int32_t> seen((size_t)m->n_tags);
  fm_prepare(*m, &b, g->h_start, g->h_lut, g->h_lay, seen.data());
  b.lay = lay;
  const size_t N = (size_t)m->n, T = (size_t)m->n_tags;
  if (m->obs_dirty) {
    HIPCHK(hipMemcpyAsync((void*)b.obs, m->obs.data(), N * sizeof(FmObs), hipMemcpyHostToDevice, g->st));
    m->obs_dirty = false;
  }
  HIPCHK(hipMemcpyAsync((void*)b.lay.lut, g->h_lut, kFpMaxIds * sizeof(int16_t), hipMemcpyHostToDevice, g->st));
  HIPCHK(hipMemcpyAsync((void*)b.lay.tags, g->h_lay, T * sizeof(FpTag), hipMemcpyHostToDevice, g->st));
  for (int q = 0; q < 2; q++)
    HIPCHK(hipMemcpyAsync(b.tag[q], g->h_start, T * sizeof(CalPose), hipMemcpyHostToDevice, g->st));
  HIPCHK(hipMemsetAsync(b.ctl, 0, sizeof(CalCtl), g->st));
  if (m->profiling) HIPCHK(hipEventRecord(g->ev[0], g->st));
  HIPCHK(launch_fieldmap(b, g->st));
  if (m->profiling) HIPCHK(hipEventRecord(g->ev[1], g->st));
  HIPCHK(hipMemcpyAsync(g->h_ctl, b.ctl, sizeof(CalCtl), hipMemcpyDeviceToHost, g->st));
  for (int q = 0; q < 2; q++) {
    HIPCHK(hipMemcpyAsync(g->h_tag[q], b.tag[q], T * sizeof(CalPose), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpyAsync(g->h_pose[q], b.pose[q], N * sizeof(CalPose), hipMemcpyDeviceToHost, g->st));
  }
  HIPCHK(hipMemcpyAsync(g->h_cov, b.cov, T * 36 * sizeof(double), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(g->h_viewcost, b.viewcost, N * sizeof(double), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(g->h_ntags, b.ntags, N * sizeof(int32_t), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  uint64_t ns = 0;
  if (m->profiling) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]));
    ns = (uint64_t)((double)ms * 1e6);
  }
  const int w = g->h_ctl->which & 1;
  fm_finish(m, b, *g->h_ctl, g->h_start, seen.data(), g->h_tag[w], g->h_cov, g->h_pose[w], g->h_viewcost, g->h_ntags,
            out);
  m->ns = ns;
  return AT_OK;
}

// ---- rig track -------------------------------------------------------------------
// The device side of an at_rigtrack (at_rigtrack.cpp holds the rest), as CalGpu: a stream and
// events of its own, the layout, the ring of stored instants and their own starts in HBM (a slot
// is uploaded, and its start computed, once per stored instant), the solve's buffers for a full
// window, and pinned host memory for what comes back.  Everything is sized by the window at the
// first solve.
namespace at {
constexpr int kTrkEvents = 3 + 2 * (kTrkMaxIters + 1);
struct TrkGpu {
  int device;
  hipStream_t st;
  hipEvent_t ev[kTrkEvents];
  bool ready;
  std::vector<void*> dev, host;
  TrkBufs b;  // device pointers
  CalPose* h_pose[2];
  double *h_instpx, *h_cov;
  int32_t* h_own_nt;
  TrkCtl* h_ctl;
};
}  // namespace at

static void trkgpu_free(TrkGpu* g) {
  if (!g) return;
  (void)hipSetDevice(g->device);
  if (g->st) (void)hipStreamSynchronize(g->st);
  for (void* p : g->dev) (void)hipFree(p);
  for (void* p : g->host) (void)hipHostFree(p);
  for (hipEvent_t e : g->ev)
    if (e) (void)hipEventDestroy(e);
  if (g->st) (void)hipStreamDestroy(g->st);
  delete g;
}

static int trkgpu_reserve(at_rigtrack* t, TrkGpu* g) {
  bool ok = true;
  auto dmal = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (!ok || hipMalloc(&p, bytes) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    g->dev.push_back(p);
    return p;
  };
  auto hmal = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (!ok || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    g->host.push_back(p);
    return p;
  };
  TrkBufs& b = g->b;
  memset(&b, 0, sizeof(b));
  const size_t W = (size_t)t->window, nc = (size_t)t->n_cams;
  b.obs = (const CalCamObs*)dmal(W * nc * sizeof(CalCamObs));
  b.odom = (const TrkOdom*)dmal(W * sizeof(TrkOdom));
  b.rec = (RigRecord*)dmal(W * sizeof(RigRecord));
  b.own = (CalPose*)dmal(W * sizeof(CalPose));
  b.own_nt = (int32_t*)dmal(W * sizeof(int32_t));
  for (int q = 0; q < 2; q++) {
    b.pose[q] = (CalPose*)dmal(W * sizeof(CalPose));
    b.sums[q] = (double*)dmal(W * kTrkSums * sizeof(double));
    g->h_pose[q] = (CalPose*)hmal(W * sizeof(CalPose));
  }
  b.instpx = (double*)dmal(W * sizeof(double));
  b.cov = (double*)dmal(36 * sizeof(double));
  b.ctl = (TrkCtl*)dmal(sizeof(TrkCtl));
  b.lay.lut = (const int16_t*)dmal(kFpMaxIds * sizeof(int16_t));
  b.lay.tags = (const FpTag*)dmal(t->tags.size() * sizeof(FpTag));
  b.lay.max_hamming = t->max_hamming;
  g->h_instpx = (double*)hmal(W * sizeof(double));
  g->h_cov = (double*)hmal(36 * sizeof(double));
  g->h_own_nt = (int32_t*)hmal(W * sizeof(int32_t));
  g->h_ctl = (TrkCtl*)hmal(sizeof(TrkCtl));
  if (!ok) return AT_E_NOMEM;
  if (hipMemcpy((void*)b.lay.lut, t->lut.data(), kFpMaxIds * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy((void*)b.lay.tags, t->tags.data(), t->tags.size() * sizeof(FpTag), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemset(b.own_nt, 0, W * sizeof(int32_t)) != hipSuccess)
    return AT_E_HIP;
  t->dev_stale.assign(W, 1);
  g->ready = true;
  return AT_OK;
}

int at_rigtrack_solve(at_rigtrack* t, at_rigtrack_result* out) {
  if (!t || !out || t->n < 1) return AT_E_INVALID;
  {  // (no kernel is launched for a window without a tag)
    bool any = false;
    for (int k = 0; k < t->n && !any; k++)
      for (int c = 0; c < t->n_cams && !any; c++)
        any = t->obs[(size_t)((t->head + k) % t->window) * t->n_cams + c].m > 0;
    if (!any) return AT_E_INVALID;
  }
  TrkGpu* g = t->gpu;
  if (!g) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AT_E_HIP;
    g = new TrkGpu();
    g->device = dev;
    bool ok = hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < kTrkEvents && ok; i++) ok = hipEventCreateWithFlags(&g->ev[i], kTimingEventFlags) == hipSuccess;
    if (!ok) {
      trkgpu_free(g);
      return AT_E_HIP;
    }
    t->gpu = g;
    t->gpu_free = trkgpu_free;
  }
  if (hipSetDevice(g->device) != hipSuccess) return AT_E_HIP;
  if (!g->ready) {
    const int rc = trkgpu_reserve(t, g);
    if (rc != AT_OK) return rc;
  }
  TrkBufs b = g->b;
  const FpLayout lay = b.lay;
  trk_fill_bufs(*t, &b);
  b.lay = lay;
  const size_t W = (size_t)t->window, N = (size_t)t->n, nc = (size_t)t->n_cams;
  TrkTodo todo;
  memset(&todo, 0, sizeof(todo));
  for (int k = 0; k < t->n; k++) {
    const int s = b.slot(k);
    if (!t->dev_stale[(size_t)s]) continue;
    HIPCHK(hipMemcpyAsync((void*)(b.obs + (size_t)s * nc), t->obs.data() + (size_t)s * nc, nc * sizeof(CalCamObs),
                          hipMemcpyHostToDevice, g->st));
    HIPCHK(hipMemcpyAsync((void*)(b.odom + s), t->odom.data() + s, sizeof(TrkOdom), hipMemcpyHostToDevice, g->st));
    todo.slot[todo.n++] = (uint8_t)s;
  }
  const int n_ev = 3 + 2 * (t->iters + 1);
  HIPCHK(launch_rigtrack(b, todo, t->iters, g->st, t->profiling ? g->ev : nullptr));
  // (a slot counts as held by the device only now: a failure above leaves it to the next solve)
  for (int i = 0; i < todo.n; i++) t->dev_stale[todo.slot[i]] = 0;
  HIPCHK(hipMemcpyAsync(g->h_ctl, b.ctl, sizeof(TrkCtl), hipMemcpyDeviceToHost, g->st));
  for (int q = 0; q < 2; q++)
    HIPCHK(hipMemcpyAsync(g->h_pose[q], b.pose[q], N * sizeof(CalPose), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(g->h_cov, b.cov, 36 * sizeof(double), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(g->h_instpx, b.instpx, N * sizeof(double), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipMemcpyAsync(g->h_own_nt, b.own_nt, W * sizeof(int32_t), hipMemcpyDeviceToHost, g->st));
  HIPCHK(hipStreamSynchronize(g->st));
  uint64_t ns[4] = {0, 0, 0, 0};
  if (t->profiling) {
    for (int i = 0; i + 1 < n_ev; i++) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, g->ev[i], g->ev[i + 1]));
      const uint64_t v = (uint64_t)((double)ms * 1e6);
      ns[0] += v;
      ns[i < 2 ? 1 : (i & 1) ? 3 : 2] += v;
    }
  }
  if (!g->h_ctl->any) return AT_E_INVALID;
  const int w = g->h_ctl->which & 1;
  trk_finish(t, *g->h_ctl, g->h_pose[w], g->h_cov, g->h_instpx, g->h_own_nt, out);
  for (int i = 0; i < 4; i++) t->ns[i] = ns[i];
  return AT_OK;
}

int at_gp_tensor(at_detector* d, int frame, const float** dev_ptr) {
  if (!d || !dev_ptr || !d->prm.gp_c || !d->last_gp || frame < 0 || frame >= d->last_nframes) return AT_E_INVALID;
  *dev_ptr = d->d.gp_out + (size_t)frame * d->prm.gp_c * d->prm.gp_w * d->prm.gp_h;
  return AT_OK;
}

int at_gp_copy(at_detector* d, int frame, float* dst, size_t count) {
  const float* src = nullptr;
  const int rc = at_gp_tensor(d, frame, &src);
  if (rc != AT_OK) return rc;
  const size_t n = (size_t)d->prm.gp_c * d->prm.gp_w * d->prm.gp_h;
  if (!dst || count < n) return AT_E_INVALID;
  if (hipSetDevice(d->device) != hipSuccess) return AT_E_HIP;
  if (d->pending && hipEventSynchronize(d->ev_done) != hipSuccess) return AT_E_HIP;
  return hipMemcpy(dst, src, n * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess ? AT_OK : AT_E_HIP;
}

int at_gp_preprocess_device(const uint8_t* bgr, int width, int height, float* out, int out_width, int out_height,
                            int channels, void* stream) {
  if (!bgr || !out || width < 2 || height < 2 || out_width < 1 || out_height < 1 || out_width > 8192 ||
      out_height > 8192 || (channels != 1 && channels != 3))
    return AT_E_INVALID;
  return launch_gp_preprocess(bgr, width, height, out, out_width, out_height, channels, (hipStream_t)stream) ==
                 hipSuccess
             ? AT_OK
             : AT_E_HIP;
}

int at_set_debug_taps(at_detector* d, int enable) {
  if (!d) return AT_E_INVALID;
  if (hipSetDevice(d->device) != hipSuccess) return AT_E_HIP;
  if (d->pending && hipEventSynchronize(d->ev_done) != hipSuccess) return AT_E_HIP;
  if (d->prm.taps != (enable ? 1 : 0)) {
    d->prm.taps = enable ? 1 : 0;
    drop_graphs(d);  // the captured sequences carry the old parameters
  }
  return AT_OK;
}

int at_frame_status(at_detector* d, int frame) {
  if (!d || frame < 0 || frame >= d->last_nframes) return AT_E_INVALID;
  if (d->mj_ent_batch && !d->pending && d->h_ent_info[(size_t)frame * at::kEntInfoWords]) return AT_E_INVALID;
  const uint32_t s = d->h_ctrl[kCtlStatus * d->B + frame];
  return (s & (kStatusPairsOverflow | kStatusHashFull | kStatusPointsOverflow | kStatusQuadsOverflow | kStatusDetsOverflow |
               kStatusPairsCapped))
             ? AT_E_CAPACITY
             : AT_OK;
}

long long at_debug_copy(at_detector* d, int stage, int frame, void* dst, size_t bytes) {
  if (!d || !dst || frame < 0 || frame >= d->last_nframes) return AT_E_INVALID;
  if (hipSetDevice(d->device) != hipSuccess) return AT_E_HIP;
  if (d->pending && hipEventSynchronize(d->ev_done) != hipSuccess) return AT_E_HIP;
  const Geom& g = d->g;
  const size_t npix = (size_t)g.W * g.H, nd = (size_t)g.Wd * g.Hd;
  const void* src = nullptr;
  size_t n = 0;
  const int B = d->B;
  std::vector<uint8_t> tmp;
  switch (stage) {
    case AT_STAGE_GRAY:
      if (!d->last_gray) return AT_E_INVALID;  // YUYV / GRAY8 batches without the debug taps
      src = d->d.gray + frame * npix; n = npix; break;
    case AT_STAGE_DECIMATED: src = d->d.dec + frame * nd; n = nd; break;
    case AT_STAGE_THRESHOLD: src = d->d.thr + frame * nd; n = nd; break;
    case AT_STAGE_LABELS: {
      // LabelImage's output (labeling_allegretti_2019_BKE.cu:340-462), resolved from
      // the union-find forest on the device (k_tap_labels)
      if (bytes < nd * 4) return AT_E_INVALID;
      uint32_t* tmp_d = nullptr;
      if (hipMalloc(&tmp_d, nd * 4) != hipSuccess) return AT_E_NOMEM;
      hipError_t e = launch_tap_labels(d->d.thr + frame * nd, d->d.par + frame * nd, tmp_d, g.Wd, g.Hd, d->st);
      if (e == hipSuccess) e = hipStreamSynchronize(d->st);
      if (e == hipSuccess) e = hipMemcpy(dst, tmp_d, nd * 4, hipMemcpyDeviceToHost);
      (void)hipFree(tmp_d);
      return e == hipSuccess ? (long long)(nd * 4) : AT_E_HIP;
    }
    case AT_STAGE_SIZES: {
      // the dense plane of the reference, masked from the forest on the device
      if (bytes < nd * 4 || !d->last_sizes) return AT_E_INVALID;
      uint32_t* tmp_d = nullptr;
      if (hipMalloc(&tmp_d, nd * 4) != hipSuccess) return AT_E_NOMEM;
      hipError_t e = launch_tap_sizes(d->d.thr + frame * nd, d->d.par + frame * nd, d->d.size + frame * nd, tmp_d,
                                      g.Wd, g.Hd, d->st);
      if (e == hipSuccess) e = hipStreamSynchronize(d->st);
      if (e == hipSuccess) e = hipMemcpy(dst, tmp_d, nd * 4, hipMemcpyDeviceToHost);
      (void)hipFree(tmp_d);
      return e == hipSuccess ? (long long)(nd * 4) : AT_E_HIP;
    }
    case AT_STAGE_NUM_POINTS:
      if (bytes < 4) return AT_E_INVALID;
      memcpy(dst, &d->h_ctrl[kCtlNpts * B + frame], 4);
      return 4;
    case AT_STAGE_NUM_PAIRS:
      if (bytes < 4) return AT_E_INVALID;
      memcpy(dst, &d->h_ctrl[kCtlNpairs * B + frame], 4);
      return 4;
    case AT_STAGE_NUM_PAIR_ENTRIES:
      if (bytes < 4) return AT_E_INVALID;
      memcpy(dst, &d->h_ctrl[kCtlNpent * B + frame], 4);
      return 4;
    case AT_STAGE_PROBE: src = d->d.probe; n = kProbeWords * 8; break;
    case AT_STAGE_QUADS: {
      // one record per kept blob, in the slot of its pair rank (pair_sel marks them),
      // written while the debug taps are on
      if (!d->prm.taps) return AT_E_INVALID;
      const uint32_t npairs = std::min<uint32_t>(d->h_ctrl[kCtlNpairs * B + frame], (uint32_t)kMaxPairs);
      std::vector<QuadRecord> all(npairs);
      std::vector<uint32_t> sel(npairs);
      if (npairs && (hipMemcpy(all.data(), d->d.quads + (size_t)frame * kMaxPairs, npairs * sizeof(QuadRecord),
                               hipMemcpyDeviceToHost) != hipSuccess ||
                     hipMemcpy(sel.data(), d->d.pair_sel + (size_t)frame * kMaxPairs, npairs * 4,
                               hipMemcpyDeviceToHost) != hipSuccess))
        return AT_E_HIP;
      std::vector<QuadRecord> q;
      for (uint32_t i = 0; i < npairs; i++)
        if (sel[i]) q.push_back(all[i]);
      const uint32_t nq = (uint32_t)q.size();
      const size_t need = nq * sizeof(at_quad_record);
      if (bytes < need) return AT_E_INVALID;
      for (uint32_t i = 0; i < nq; i++) {
        at_quad_record r;
        r.blob_index = q[i].blob_index;
        r.valid = q[i].valid;
        r.accepted = q[i].accepted;
        memcpy(r.indices, q[i].indices, sizeof(r.indices));
        memcpy(r.corners, q[i].corners, sizeof(r.corners));
        memcpy((uint8_t*)dst + i * sizeof(at_quad_record), &r, sizeof(r));
      }
      return (long long)need;
    }
    case AT_STAGE_POINTS: {
      // the tiles' regions concatenated in tile order
      const size_t ntb = (size_t)g.ntb;
      std::vector<uint32_t> tc(ntb);
      std::vector<uint64_t> all(ntb * (size_t)g.bnd_region);
      if (hipMemcpy(tc.data(), d->d.tcnt + frame * ntb, ntb * 4, hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(all.data(), d->d.pts + frame * ntb * g.bnd_region, all.size() * 8, hipMemcpyDeviceToHost) !=
              hipSuccess)
        return AT_E_HIP;
      size_t np = 0;
      for (size_t t = 0; t < ntb; t++) np += tc[t] & ~kTileNarrow;
      if (bytes < np * 8) return AT_E_INVALID;
      // narrow tiles hold (entry index, point bits) words: the key is the entry's pair
      // key over the point bits
      std::vector<uint64_t> ekey(ntb * (size_t)kLdsPairSlots);
      if (hipMemcpy(ekey.data(), d->d.pent_key + frame * ntb * kLdsPairSlots, ekey.size() * 8,
                    hipMemcpyDeviceToHost) != hipSuccess)
        return AT_E_HIP;
      // the device keys pairs by node index (node_F / node_L: three words per 2x2 block,
      // monotone in the node id); the reference's QuadBoundaryPoint carries the node ids
      auto node_id = [&](uint64_t n) -> uint64_t {
        const uint64_t P = 3 * (uint64_t)g.BW, by = n / P, r = n - by * P;
        return r < (uint64_t)g.BW ? 2 * by * g.Wd + 2 * r : (2 * by + 1) * g.Wd + (r - g.BW);
      };
      auto to_ref = [&](uint64_t k) -> uint64_t {
        return (node_id(k >> 44) << 44) | (node_id((k >> 24) & 0xfffff) << 24) | (k & 0xffffffu);
      };
      size_t o = 0;
      for (size_t t = 0; t < ntb; t++) {
        const uint32_t n = tc[t] & ~kTileNarrow;
        if (tc[t] & kTileNarrow) {
          const uint32_t* w = reinterpret_cast<const uint32_t*>(all.data() + t * g.bnd_region);
          for (uint32_t i = 0; i < n; i++) {
            const uint64_t key =
                to_ref((ekey[t * kLdsPairSlots + (w[i] >> 23)] << 24) | ((w[i] & 0x7ffffcu) << 1) | (w[i] & 3u));
            memcpy((uint8_t*)dst + (o + i) * 8, &key, 8);
          }
        } else {
          for (uint32_t i = 0; i < n; i++) {
            const uint64_t key = to_ref(all[t * g.bnd_region + i]);
            memcpy((uint8_t*)dst + (o + i) * 8, &key, 8);
          }
        }
        o += n;
      }
      return (long long)(np * 8);
    }
    case AT_STAGE_BLOB_POINTS: {
      // IndexPoint keys of the selected pairs, in rank order (written by the blob
      // kernels only while the debug taps are on)
      if (!d->prm.taps) return AT_E_INVALID;
      const uint32_t npairs = std::min<uint32_t>(d->h_ctrl[kCtlNpairs * B + frame], (uint32_t)kMaxPairs);
      std::vector<uint32_t> cnt(npairs), off(npairs), sel(npairs);
      if (npairs) {
        if (hipMemcpy(cnt.data(), d->d.pair_cnt + (size_t)frame * kMaxPairs, npairs * 4, hipMemcpyDeviceToHost) ||
            hipMemcpy(off.data(), d->d.pair_off + (size_t)frame * kMaxPairs, npairs * 4, hipMemcpyDeviceToHost) ||
            hipMemcpy(sel.data(), d->d.pair_sel + (size_t)frame * kMaxPairs, npairs * 4, hipMemcpyDeviceToHost))
          return AT_E_HIP;
      }
      size_t total = 0;
      for (uint32_t i = 0; i < npairs; i++)
        if (sel[i]) total += cnt[i];
      if (bytes < total * 8) return (long long)(total * 8);
      size_t o = 0;
      for (uint32_t i = 0; i < npairs; i++) {
        if (!sel[i]) continue;
        if (hipMemcpy((uint8_t*)dst + o * 8, d->d.keys + (size_t)frame * g.cap_pts + off[i], cnt[i] * 8,
                      hipMemcpyDeviceToHost) != hipSuccess)
          return AT_E_HIP;
        o += cnt[i];
      }
      return (long long)(total * 8);
    }
    default: return AT_E_INVALID;
  }
  if (bytes < n) return AT_E_INVALID;
  if (n && hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) return AT_E_HIP;
  return (long long)n;
}

}  // extern "C"
