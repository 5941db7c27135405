// at_rigrobust.h -- the rig pose with Huber weights and bad-tag rejection, shared by host and
// device.
//
// at_rigpose.h's solve is plain least squares: one wrong tag (a layout tag bumped on the field, a
// false decode, a corner dragged by glare) pulls the fused robot pose with it.  Here every corner
// costs the Huber function of its reprojection error, and after the fit whole tags whose error
// stays large are dropped and the fit is run again, a few rounds at most.
//
// With s = ru^2 + rv^2 the squared reprojection error of a corner and k = huber_px:
//   s <= k k:   rho = s,                  w = 1
//   otherwise:  rho = 2 k sqrt(s) - k k,  w = k / sqrt(s)
// and a corner with Pz <= 0 has s = HUGE_VAL, as in at_rigpose.h.  The cost is the sum of rho; the
// normal equations are each slot's 27 values of rig_slot_normal times its w at the linearisation
// point (iteratively reweighted least squares inside the same Levenberg-Marquardt loop, lambda
// schedule and accept rule `ok && cn < cost`).  The slots of a dropped tag are marked invalid and
// add +0.0 to every sum, like unused slots.
//
// A rejection round, at the current pose: per kept tag S = (s0 + s1) + (s2 + s3) over its four
// corners; a tag with S > 4 reject_px^2 (an RMS beyond reject_px) is a candidate.  Each camera's
// wave leader stores its candidate and kept counts in RigRobustShared, one barrier, every thread
// adds them in camera order: no candidate ends the loop; candidates that would leave fewer than
// min_keep tags end it with starved = 1 and nothing dropped; otherwise all candidates are dropped
// and the fit runs again from the current pose with lambda back at 1e-3.  Every thread reads the
// decision from the same LDS words after the same barrier, so every branch around a barrier is
// uniform over the workgroup (k_rig's rule); instants may run different numbers of rounds.
//
// Results: one last pass sums w s and s over the kept slots; rms_px = sqrt(sum s / (4 n_kept)),
// cov = sum w s / (8 n_kept - 6) times the inverse of the weighted J^T W J, and per selected tag,
// dropped or not, tag_rms_px = sqrt(S / 4) at the final pose.  n_tags, tags_per_cam and ids of the
// record are the selection, as in the plain solve; steps_taken and rejected count over all fits.
//
// at_rigpose.h's rules hold: no contraction, only + - * / sqrt, the 64-slot tree per camera and
// then ((c0 + c1) + c2) + .. through RigShared.  With huber_px = reject_px = +inf every w is 1.0,
// which multiplies exactly, rho is s and no tag is a candidate: the record is the plain solve's bit
// for bit (while the projected start has a finite cost, the only case in which the plain solve's
// rms_px is not the sum at the final pose).
//
// Limits: the test is on a tag's error under a pose that the bad tag itself helped to fit.  A small
// displacement among few tags is absorbed by the pose and not detected (2 cm in a one-camera view
// of three tags is not), and a majority of bad tags drags the fit to themselves: the good ones are
// then the ones dropped.
//
// The team is at_rigpose.h's plus tag_sum(s, S) -- every slot's S of its tag: lane xor 1, then
// xor 2 --, tag_mask(f): bit j set where f holds in slot 4 j, and count(f): the camera's slots
// in which f holds.
#pragma once

#include "at_rigpose.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace at {

constexpr int kRigMaxRounds = 3;

// at_rig_robust_config
struct RigRobustCfg {
  double huber_px, reject_px;
  int32_t max_rounds, min_keep;
};
static_assert(sizeof(RigRobustCfg) == 24, "RigRobustCfg: 24 B");

// at_rig_robust_info
struct RigRobustInfo {
  int32_t n_kept, n_rejected, rounds, starved;
  uint32_t rejected_mask[kRigMaxCams];
  double tag_rms_px[kRigMaxCams][kFpMaxTags];
  double huber_cost;
  int32_t n_downweighted, pad;
};
static_assert(sizeof(RigRobustInfo) == 1088, "RigRobustInfo: 1088 B per instant");

struct RigRobustShared {
  RigShared base;
  int32_t cand[kRigMaxCams];  // per camera: candidates of this round,
  int32_t kept[kRigMaxCams];  // tags still kept before it,
  int32_t down[kRigMaxCams];  // kept corners beyond huber_px at the final pose
};

AT_FP_HD bool rig_robust_cfg_ok(const RigRobustCfg& c) {
  return c.huber_px > 0.0 && c.reject_px > 0.0 && c.max_rounds >= 0 && c.max_rounds <= kRigMaxRounds &&
         c.min_keep >= 1;
}

AT_FP_HD void rig_huber(double s, double k, double kk, double* rho, double* w) {
  if (s <= kk) {
    *rho = s;
    *w = 1.0;
  } else {
    const double e = sqrt(s);
    *rho = (2.0 * k) * e - kk;
    *w = k / e;
  }
}

AT_FP_HD int rig_popcount(uint32_t m) {
  int n = 0;
  for (int j = 0; j < kFpMaxTags; j++) n += (int)((m >> j) & 1u);
  return n;
}

// summed rho of all slots of all cameras under (R, t)
template <class T>
AT_FP_HD double rig_robust_cost(const T& tm, RigShared& sh, int* phase, int n_cams, FpSlot (*slots)[T::NS],
                                const RigCam* cams, const double* R, const double* t, double k, double kk) {
  const int buf = rig_next_buf<T>(phase);
  for (int c = 0; c < T::NC; c++) {
    if (tm.cam(c) >= n_cams) continue;
    double e[T::NS][1];
#pragma unroll
    for (int s = 0; s < T::NS; s++) {
      double w;
      rig_huber(rig_slot_cost(slots[c][s], cams[c], R, t), k, kk, &e[s][0], &w);
    }
    rig_put<1>(tm, sh, buf, c, e);
  }
  double v;
  rig_get<1>(tm, sh, buf, n_cams, &v);
  return v;
}

// the weighted normal equations at (R, t) into o[27]
template <class T>
AT_FP_HD void rig_robust_normal(const T& tm, RigShared& sh, int* phase, int n_cams, FpSlot (*slots)[T::NS],
                                const RigCam* cams, const double* R, const double* t, double k, double kk, double* o) {
  const int buf = rig_next_buf<T>(phase);
  for (int c = 0; c < T::NC; c++) {
    if (tm.cam(c) >= n_cams) continue;
    double ps[T::NS][27];
#pragma unroll
    for (int s = 0; s < T::NS; s++) {
      rig_slot_normal(slots[c][s], cams[c], R, t, ps[s]);
      double rho, w;
      rig_huber(rig_slot_cost(slots[c][s], cams[c], R, t), k, kk, &rho, &w);
#pragma unroll
      for (int i = 0; i < 27; i++) ps[s][i] = ps[s][i] * w;
    }
    rig_put<27>(tm, sh, buf, c, ps);
  }
  rig_get<27>(tm, sh, buf, n_cams, o);
}

// kFpIters Levenberg-Marquardt iterations from (R, t) of cost *cost, lambda from 1e-3
template <class T>
AT_FP_HD void rig_robust_fit(const T& tm, RigShared& sh, int* phase, int n_cams, FpSlot (*slots)[T::NS],
                             const RigCam* cams, double k, double kk, double* R, double* t, double* cost, int* steps,
                             int* rejected) {
  double lambda = 1e-3;
  for (int it = 0; it < kFpIters; it++) {
    double ag[27];
    rig_robust_normal(tm, sh, phase, n_cams, slots, cams, R, t, k, kk, ag);
    double d[6], Rn[9], tn[3];
    const bool ok = fp_solve6(ag, ag + 21, lambda, d);
    if (!ok)
      for (int i = 0; i < 6; i++) d[i] = 0.0;
    rig_apply_step(R, t, d, Rn, tn);
    const double cn = rig_robust_cost(tm, sh, phase, n_cams, slots, cams, Rn, tn, k, kk);
    if (ok && cn < *cost) {
      for (int i = 0; i < 9; i++) R[i] = Rn[i];
      for (int i = 0; i < 3; i++) t[i] = tn[i];
      *cost = cn;
      *steps = *steps + 1;
      lambda = lambda / 10.0;
      if (lambda < 1e-9) lambda = 1e-9;
    } else {
      *rejected = *rejected + 1;
      lambda = lambda * 10.0;
    }
  }
}

// Team, Src: rig_solve_instant's, the team with tag_sum and tag_mask.  Every thread ends with the
// same record and the same scalars of the info; the leader stores them to out / info (and out2 /
// info2 when given), and each camera's wave stores its own row of tag_rms_px and rejected_mask.
template <class T, class Src>
AT_FP_HD void rig_solve_instant_robust(const T& tm, const Src& src, RigRobustShared& rx, const FpLayout& lay,
                                       int n_cams, double tag_size, const RigRobustCfg& cfg, RigRecord* out,
                                       RigRecord* out2, RigRobustInfo* info, RigRobustInfo* info2) {
  RigShared& sh = rx.base;
  const double hk = cfg.huber_px, kk = hk * hk;
  const double cut = 4.0 * cfg.reject_px * cfg.reject_px;

  // ---- per camera: select, points, each tag's own pose as a robot pose (rig_solve_instant's) ----
  FpSlot slots[T::NC][T::NS];
  bool sel[T::NC][T::NS];  // the selection: slots[][].valid before any tag was dropped
  RigCam cams[T::NC];
  uint32_t gone[T::NC];    // bit j: this camera's j-th tag was dropped
  for (int k = 0; k < T::NC; k++) {
    gone[k] = 0;
    const int ci = tm.cam(k);
    if (ci >= n_cams) continue;
    const auto cs = src.cam(ci);
    cams[k] = src.rigcam(ci);
    uint32_t my_cand[T::NS], my_id[T::NS];
    int m, dropped;
    fp_select(tm.wave(), cs, lay, my_cand, my_id, &m, &dropped);
    fp_points(tm.wave(), cs, lay, tag_size, m, my_cand, my_id, slots[k]);
#pragma unroll
    for (int s = 0; s < T::NS; s++) sel[k][s] = slots[k][s].valid;
    for (int j = 0; j < m; j++) {
      const int c = (int)tm.wave().from_slot(my_cand, 4 * j);
      const uint32_t id = tm.wave().from_slot(my_id, 4 * j);
      const FpTag& tg = lay.tags[lay.lut[id]];
      double Rfc[9], tfc[3], rt[3], Rj[9], re[3];
      fp_mul_abt(tg.R, cs.pose_R(c), Rfc);
      fp_rot(Rfc, cs.pose_t(c), rt);
      for (int i = 0; i < 3; i++) tfc[i] = tg.t[i] - rt[i];
      fp_mul_abt(Rfc, cams[k].ER, Rj);
      fp_rot(Rj, cams[k].Et, re);
      if (tm.wave_leader()) {
        for (int i = 0; i < 9; i++) sh.cand[ci][j][i] = Rj[i];
        for (int i = 0; i < 3; i++) sh.cand[ci][j][9 + i] = tfc[i] - re[i];
        sh.ids[ci][j] = (int32_t)id;
      }
    }
    if (tm.wave_leader()) {
      sh.m[ci] = m;
      sh.dropped[ci] = dropped;
    }
  }
  tm.barrier();
  int n_tags = 0, n_used = 0, dropped = 0;
  for (int i = 0; i < n_cams; i++) {
    n_tags += sh.m[i];
    n_used += sh.m[i] > 0;
    dropped += sh.dropped[i];
  }

  // ---- start: the single-tag pose with the least summed rho ----
  int phase = 0;
  double R[9], t[3];
  double cost = HUGE_VAL;
  bool found = false;
  for (int i = 0; i < n_cams; i++) {
    const int mi = sh.m[i];
    for (int j0 = 0; j0 < mi; j0 += kRigChunk) {
      const int buf = rig_next_buf<T>(&phase);
      for (int k = 0; k < T::NC; k++) {
        if (tm.cam(k) >= n_cams) continue;
        double e[T::NS][kRigChunk];
#pragma unroll
        for (int q = 0; q < kRigChunk; q++) {
          const bool have = j0 + q < mi;
          const double* cd = sh.cand[i][have ? j0 + q : j0];
#pragma unroll
          for (int s = 0; s < T::NS; s++) {
            double w;
            e[s][q] = 0.0;
            if (have) rig_huber(rig_slot_cost(slots[k][s], cams[k], cd, cd + 9), hk, kk, &e[s][q], &w);
          }
        }
        rig_put<kRigChunk>(tm, sh, buf, k, e);
      }
      double tot[kRigChunk];
      rig_get<kRigChunk>(tm, sh, buf, n_cams, tot);
#pragma unroll
      for (int q = 0; q < kRigChunk; q++)
        if (j0 + q < mi && tot[q] < cost) {
          cost = tot[q];
          found = true;
          const double* cd = sh.cand[i][j0 + q];
          for (int e = 0; e < 9; e++) R[e] = cd[e];
          for (int e = 0; e < 3; e++) t[e] = cd[9 + e];
        }
    }
  }
  if (!found) {
    if (tm.leader()) {
      RigRecord z = {};
      z.dropped = dropped;
      const RigRobustInfo zi = {};
      *out = z;
      *info = zi;
      if (out2) *out2 = z;
      if (info2) *info2 = zi;
    }
    return;
  }
  fp_project_rotation(R);
  {
    const double c0 = rig_robust_cost(tm, sh, &phase, n_cams, slots, cams, R, t, hk, kk);
    if (c0 < HUGE_VAL) cost = c0;
  }

  // ---- fit, then rounds of: drop the tags whose error stays beyond reject_px, fit again ----
  int steps = 0, rejected = 0, rounds = 0, starved = 0, n_kept = n_tags;
  rig_robust_fit(tm, sh, &phase, n_cams, slots, cams, hk, kk, R, t, &cost, &steps, &rejected);
  for (int r = 0; r < cfg.max_rounds; r++) {
    uint32_t cm[T::NC];
    for (int k = 0; k < T::NC; k++) {
      cm[k] = 0;
      const int ci = tm.cam(k);
      if (ci >= n_cams) continue;
      double e[T::NS], S[T::NS];
      bool kf[T::NS], cf[T::NS];
#pragma unroll
      for (int s = 0; s < T::NS; s++) e[s] = rig_slot_cost(slots[k][s], cams[k], R, t);
      tm.tag_sum(e, S);
#pragma unroll
      for (int s = 0; s < T::NS; s++) {
        kf[s] = slots[k][s].valid;
        cf[s] = kf[s] && S[s] > cut;
      }
      cm[k] = tm.tag_mask(cf);
      const uint32_t km = tm.tag_mask(kf);
      if (tm.wave_leader()) {
        rx.cand[ci] = rig_popcount(cm[k]);
        rx.kept[ci] = rig_popcount(km);
      }
    }
    tm.barrier();
    int nc = 0, nk = 0;
    for (int i = 0; i < n_cams; i++) {
      nc += rx.cand[i];
      nk += rx.kept[i];
    }
    if (nc == 0) break;
    if (nk - nc < cfg.min_keep) {
      starved = 1;
      break;
    }
    for (int k = 0; k < T::NC; k++) {
      gone[k] |= cm[k];
#pragma unroll
      for (int s = 0; s < T::NS; s++)
        if ((cm[k] >> (tm.wave().slot(s) >> 2)) & 1u) slots[k][s].valid = false;
    }
    n_kept = nk - nc;
    rounds++;
    // (the cost of the pose under the tags that are left; its barrier also parts this round's
    // reads of cand / kept from the next round's stores)
    cost = rig_robust_cost(tm, sh, &phase, n_cams, slots, cams, R, t, hk, kk);
    rig_robust_fit(tm, sh, &phase, n_cams, slots, cams, hk, kk, R, t, &cost, &steps, &rejected);
  }

  // ---- the last pass: sum w s and sum s over the kept slots, the corners beyond huber_px ----
  double fin[2];
  int n_down = 0;
  {
    const int buf = rig_next_buf<T>(&phase);
    for (int k = 0; k < T::NC; k++) {
      const int ci = tm.cam(k);
      if (ci >= n_cams) continue;
      double e[T::NS][2];
      bool df[T::NS];
#pragma unroll
      for (int s = 0; s < T::NS; s++) {
        const double q = rig_slot_cost(slots[k][s], cams[k], R, t);
        double rho, w;
        rig_huber(q, hk, kk, &rho, &w);
        e[s][0] = w * q;
        e[s][1] = q;
        df[s] = slots[k][s].valid && q > kk;
      }
      const int nd = tm.count(df);
      if (tm.wave_leader()) rx.down[ci] = nd;
      rig_put<2>(tm, sh, buf, k, e);
    }
    rig_get<2>(tm, sh, buf, n_cams, fin);
    for (int i = 0; i < n_cams; i++) n_down += rx.down[i];
  }
  const double rms = sqrt(fin[1] / (double)(4 * n_kept));

  // ---- covariance: sum w s / (8 n_kept - 6) times (J^T W J)^-1 at the final pose ----
  double cov[36];
  bool cov_ok = true;
  {
    double ag[27];
    rig_robust_normal(tm, sh, &phase, n_cams, slots, cams, R, t, hk, kk, ag);
    const double s2 = fin[0] / (double)(8 * n_kept - 6);
#pragma unroll
    for (int k = 0; k < 6; k++) {
      double rhs[6], x[6];
#pragma unroll
      for (int i = 0; i < 6; i++) rhs[i] = i == k ? -1.0 : -0.0;
      if (!fp_solve6(ag, rhs, 0.0, x)) cov_ok = false;
#pragma unroll
      for (int i = 0; i < 6; i++) cov[k * 6 + i] = s2 * x[i];
    }
  }

  // ---- every selected tag's RMS at the final pose, dropped ones too: each wave its own row ----
  for (int k = 0; k < T::NC; k++) {
    const int ci = tm.cam(k);
    if (ci >= n_cams) continue;
    double e[T::NS], S[T::NS];
#pragma unroll
    for (int s = 0; s < T::NS; s++) {
      FpSlot q = slots[k][s];
      q.valid = sel[k][s];
      e[s] = rig_slot_cost(q, cams[k], R, t);
    }
    tm.tag_sum(e, S);
#pragma unroll
    for (int s = 0; s < T::NS; s++) {
      const int sl = tm.wave().slot(s);
      if (sl & 3) continue;
      const double v = sel[k][s] ? sqrt(S[s] / 4.0) : 0.0;
      info->tag_rms_px[ci][sl >> 2] = v;
      if (info2) info2->tag_rms_px[ci][sl >> 2] = v;
    }
    if (tm.wave_leader()) {
      info->rejected_mask[ci] = gone[k];
      if (info2) info2->rejected_mask[ci] = gone[k];
    }
  }

  // ---- the record and the rest of the info ----
  if (tm.leader()) {
    for (int q = 0; q < 2; q++) {
      RigRecord* o = q ? out2 : out;
      if (!o) continue;
      o->n_tags = n_tags;
      o->n_cams_used = n_used;
      for (int i = 0; i < kRigMaxCams; i++) {
        const int mi = i < n_cams ? sh.m[i] : 0;
        o->tags_per_cam[i] = mi;
        for (int j = 0; j < kFpMaxTags; j++) o->ids[i][j] = j < mi ? sh.ids[i][j] : 0;
      }
      for (int i = 0; i < 9; i++) o->R[i] = R[i];
      for (int i = 0; i < 3; i++) o->t[i] = t[i];
#pragma unroll
      for (int i = 0; i < 36; i++) o->cov[i] = cov_ok ? cov[i] : 0.0;
      o->rms_px = rms;
      o->cov_valid = cov_ok ? 1 : 0;
      o->steps_taken = steps;
      o->rejected = rejected;
      o->dropped = dropped;
    }
    for (int q = 0; q < 2; q++) {
      RigRobustInfo* o = q ? info2 : info;
      if (!o) continue;
      o->n_kept = n_kept;
      o->n_rejected = n_tags - n_kept;
      o->rounds = rounds;
      o->starved = starved;
      for (int i = n_cams; i < kRigMaxCams; i++) {
        o->rejected_mask[i] = 0;
        for (int j = 0; j < kFpMaxTags; j++) o->tag_rms_px[i][j] = 0.0;
      }
      o->huber_cost = cost;
      o->n_downweighted = n_down;
      o->pad = 0;
    }
  }
}

// RigHostTeam with the two tag operations: every slot of every camera held by one host thread.
struct RigRobustHostTeam : RigHostTeam {
  void tag_sum(const double* s, double* S) const {
    for (int j = 0; j < kFpMaxTags; j++) {
      const double v = (s[4 * j] + s[4 * j + 1]) + (s[4 * j + 2] + s[4 * j + 3]);
      for (int c = 0; c < 4; c++) S[4 * j + c] = v;
    }
  }
  uint32_t tag_mask(const bool* f) const {
    uint32_t m = 0;
    for (int j = 0; j < kFpMaxTags; j++) m |= (uint32_t)(f[4 * j] ? 1u : 0u) << j;
    return m;
  }
  int count(const bool* f) const {
    int n = 0;
    for (int s = 0; s < kFpSlots; s++) n += f[s] ? 1 : 0;
    return n;
  }
};

}  // namespace at
