// ba_batch_pack.hpp — host-only packing of the batch entry points
// (csrc/ba_batch.hip): the error type, the section layout of a staging buffer,
// the CSR-offset validation, the summary record, and per entry point a
// check_* (everything the kernels index with or branch on) and a *_layout (the
// sections of its staging buffer):
//   ba_prune, ba_solve_pose_batch, ba_triangulate,
//   ba_pnp_ransac, ba_two_view_ransac and their inspection entries,
//   ba_match_descriptors, ba_map_points_update, ba_associate,
//   ba_map_graph (with its plain restatement), ba_icp (with its grid plan),
//   ba_solve_window_batch (with its structure build).
// It indexes with caller-supplied arrays, so it is plain C++17 without a HIP
// header and runs under ASan + UBSan (tests/cpp/batch_pack.cpp,
// `make -C tests/cpp sanitize`).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ba_hip.h"
#include "../csrc/ba_icp.h"
#include "../csrc/ba_map_graph.h"

namespace bahip {

struct BaError { int code; std::string msg; };

// Offsets of the sections of one staging buffer, each rounded up to `align`
// bytes (a power of two): inputs (uploaded) | outputs (downloaded) | scratch.
struct SectionLayout {
  explicit SectionLayout(size_t align) : mask(align - 1) {}
  size_t add(size_t bytes) { const size_t off = total; total += (bytes + mask) & ~mask; return off; }
  void end_inputs() { in_b = total; }
  void end_outputs() { io_b = total; }
  const size_t mask;
  size_t in_b = 0, io_b = 0, total = 0;   // end of the inputs, of inputs + outputs, of everything
};

// off[0 .. n] is a CSR offset array: starts at 0 and never decreases
inline void check_offsets(const char* fn, const char* name, const int32_t* off, int n, const char* unit = "problem") {
  if (off[0] != 0) throw BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + name + "[0] != 0"};
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i])
      throw BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + name + " decreases at " + unit + " " + std::to_string(i)};
}

// The device summary record (initial cost, final cost, iterations, successful, unsuccessful,
// termination, ...) as a ba_summary; split_times: the call's wall time in all three time fields.
inline ba_summary unpack_summary(const double* rec, double wall, bool split_times) {
  ba_summary S{};
  S.initial_cost = rec[0]; S.final_cost = rec[1];
  S.num_iterations = (int)rec[2]; S.num_successful_steps = (int)rec[3]; S.num_unsuccessful_steps = (int)rec[4];
  S.termination_type = (int)rec[5];
  S.total_time_s = wall;
  if (split_times) S.linearize_time_s = S.solve_time_s = wall;
  return S;
}

// (static, here and below: a function of this header that the library's one
// user does not inline would otherwise appear among its dynamic symbols)
//
// The index / hypothesis-range check of the inspection entries
// (ba_pnp_hypotheses, ba_two_view_hypotheses, ba_two_view_hypotheses_e5):
// `what` ("problem" / "pair") index in [0, count), hypotheses [h0, h0 + n)
// inside max_hypotheses.
static inline void check_hypothesis_range(const char* fn, const char* what, int index, int count, int h0, int n, int max_hypotheses) {
  if (index < 0 || index >= count)
    throw BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what + " " + std::to_string(index) + " out of range"};
  if (h0 < 0 || n < 0 || (long long)h0 + n > max_hypotheses)
    throw BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + "hypotheses [" + std::to_string(h0) + ", " +
                                               std::to_string((long long)h0 + n) + ") outside max_hypotheses " +
                                               std::to_string(max_hypotheses)};
}

// ---------------------------------------------------------------------------
// ba_prune
// ---------------------------------------------------------------------------
static inline void check_prune(const ba_prune_problem* p, const uint8_t* result) {
  if (!p || p->n_cams < 0 || p->n_obs < 0) throw BaError{BA_ERR_INVALID_ARGUMENT, "ba_prune: bad sizes"};
  if (p->n_obs == 0) return;
  if (!p->extr || !p->cam_center || !p->K || !p->obs_cam || !p->obs_X || !p->obs_uv || !p->obs_inv_sigma ||
      !p->obs_dist || !result)
    throw BaError{BA_ERR_INVALID_ARGUMENT, "ba_prune: null array"};
  for (int o = 0; o < p->n_obs; ++o)
    if (p->obs_cam[o] < 0 || p->obs_cam[o] >= p->n_cams)
      throw BaError{BA_ERR_INVALID_ARGUMENT, "ba_prune: obs_cam[" + std::to_string(o) + "] out of range"};
}

// The staging buffer: cameras (16 + 3 + 9 floats) then pairs (1 int + 3 + 2 +
// 1 + 2 floats) | one result byte per pair.  Packed: every section is a
// multiple of its element size.
struct PruneLayout {
  SectionLayout L{1};
  size_t extr = 0, ctr = 0, K = 0, X = 0, uv = 0, sig = 0, dist = 0, cam = 0;
  size_t res = 0;
};
static inline PruneLayout prune_layout(size_t NC, size_t NO) {
  PruneLayout P;
  SectionLayout& L = P.L;
  P.extr = L.add(sizeof(float) * 16 * NC); P.ctr = L.add(sizeof(float) * 3 * NC); P.K = L.add(sizeof(float) * 9 * NC);
  P.X = L.add(sizeof(float) * 3 * NO); P.uv = L.add(sizeof(float) * 2 * NO); P.sig = L.add(sizeof(float) * NO);
  P.dist = L.add(sizeof(float) * 2 * NO); P.cam = L.add(sizeof(int32_t) * NO);
  L.end_inputs();
  P.res = L.add(NO);
  L.end_outputs();
  return P;
}

// ---------------------------------------------------------------------------
// ba_solve_pose_batch
// ---------------------------------------------------------------------------
static inline void check_pose_batch(const char* fn, const ba_pose_batch* b, const double* cams_out) {
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what}; };
  if (!b || b->n_problems < 0) throw invalid("bad batch");
  const int n = b->n_problems;
  if (n == 0) return;
  if (!b->obs_offset || !b->cams || !b->K || !cams_out) throw invalid("null array");
  check_offsets(fn, "obs_offset", b->obs_offset, n);
  if (b->obs_offset[n] > 0 && (!b->pts || !b->obs_uv)) throw invalid("null array");
}

// The staging buffer, 16-B aligned sections: the batch | poses, summary records
struct PoseLayout {
  SectionLayout L{16};
  size_t off = 0, cam = 0, K = 0, X = 0, uv = 0;
  size_t out = 0, summ = 0;
};
static inline PoseLayout pose_layout(size_t N, size_t NO) {
  PoseLayout P;
  SectionLayout& L = P.L;
  P.off = L.add(sizeof(int32_t) * (N + 1)); P.cam = L.add(sizeof(double) * 6 * N); P.K = L.add(sizeof(float) * 9 * N);
  P.X = L.add(sizeof(double) * 3 * NO); P.uv = L.add(sizeof(float) * 2 * NO);
  L.end_inputs();
  P.out = L.add(sizeof(double) * 6 * N); P.summ = L.add(sizeof(double) * 8 * N);
  L.end_outputs();
  return P;
}

// ---------------------------------------------------------------------------
// ba_triangulate
// ---------------------------------------------------------------------------
constexpr int kTriRec = 64;        // doubles per camera of the scratch: value-only record [0, 48), K-folded table [48, 64)

static inline void tri_defaults(ba_tri_options& o) {
  o.init = BA_TRI_INIT_DLT; o.refine = 0; o.min_views = 2;
  o.checks = BA_TRI_CHECK_CHEIRALITY | BA_TRI_CHECK_CHI2 | BA_TRI_CHECK_SCALE;
  o.behind_rule = 0; o.reserved = 0;
}

// Everything the kernels index with or branch on, checked on the host: the
// options (returned with the defaults applied), with refine the resolved LM
// options, then the batch and the output arrays.
static inline ba_tri_options check_triangulate(const char* fn, const ba_tri_batch* b, const ba_tri_options* topt, const ba_options& lm,
                                        const double* pts_out, const uint8_t* status) {
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what}; };
  if (!b || b->n_pts < 0 || b->n_cams < 0) throw invalid("bad batch");
  ba_tri_options t;
  if (topt) t = *topt; else tri_defaults(t);
  if (t.init != BA_TRI_INIT_DLT && t.init != BA_TRI_INIT_GIVEN) throw invalid("unknown init " + std::to_string(t.init));
  if (t.refine != 0 && t.refine != 1) throw invalid("unknown refine " + std::to_string(t.refine));
  if (t.behind_rule != 0 && t.behind_rule != 1) throw invalid("unknown behind_rule " + std::to_string(t.behind_rule));
  const int all_checks = BA_TRI_CHECK_CHEIRALITY | BA_TRI_CHECK_CHI2 | BA_TRI_CHECK_SCALE;
  if (t.checks & ~all_checks) throw invalid("unknown checks bits " + std::to_string(t.checks));
  if (t.min_views < 0) throw invalid("min_views " + std::to_string(t.min_views) + " is negative");
  if (t.refine) {
    if (lm.linear_solver != BA_DENSE_SCHUR) throw invalid("linear_solver must be BA_DENSE_SCHUR");
    if (lm.precision != BA_FP64) throw invalid("precision must be BA_FP64");
  }
  const int np = b->n_pts, nc = b->n_cams;
  if (np == 0) return t;
  if (!b->obs_offset) throw invalid("null obs_offset");
  if (!pts_out || !status) throw invalid("null output array");
  check_offsets(fn, "obs_offset", b->obs_offset, np, "point");
  const size_t no = (size_t)b->obs_offset[np];
  if (no > 0 && (!b->obs_cam || !b->obs_uv)) throw invalid("null observation array");
  if (nc > 0 && (!b->extr || !b->K)) throw invalid("null camera array (extr, K)");
  if (nc > (int)(0x7fffffff / kTriRec)) throw invalid("too many cameras");
  if (t.init == BA_TRI_INIT_GIVEN && !b->pts_init) throw invalid("init is BA_TRI_INIT_GIVEN but pts_init is null");
  if ((t.checks & BA_TRI_CHECK_SCALE) && no > 0 && !b->cam_center) throw invalid("the scale test is on but cam_center is null");
  for (size_t k = 0; k < no; ++k)
    if (b->obs_cam[k] < 0 || b->obs_cam[k] >= nc)
      throw invalid("obs_cam[" + std::to_string(k) + "] = " + std::to_string(b->obs_cam[k]) + " out of range (" +
                    std::to_string(nc) + " cameras)");
  return t;
}

// The staging buffer: cameras, offsets, observations, the optional scales and
// initial points | points, summary records, status | the camera records
struct TriLayout {
  SectionLayout L{256};
  size_t extr = 0, ctr = 0, K = 0, off = 0, oc = 0, uv = 0, sc = 0, init = 0;
  size_t pts = 0, summ = 0, st = 0;
  size_t rec = 0;
};
static inline TriLayout tri_layout(size_t nc, size_t np, size_t no, bool has_ctr, bool has_scale, bool given) {
  TriLayout P;
  SectionLayout& L = P.L;
  P.extr = L.add(sizeof(float) * 16 * nc); P.ctr = L.add(has_ctr ? sizeof(float) * 3 * nc : 0);
  P.K = L.add(sizeof(float) * 9 * nc); P.off = L.add(sizeof(int32_t) * (np + 1)); P.oc = L.add(sizeof(int32_t) * no);
  P.uv = L.add(sizeof(float) * 2 * no); P.sc = L.add(has_scale ? sizeof(float) * no : 0);
  P.init = L.add(given ? sizeof(double) * 3 * np : 0);
  L.end_inputs();
  P.pts = L.add(sizeof(double) * 3 * np); P.summ = L.add(sizeof(double) * 6 * np); P.st = L.add(np);
  L.end_outputs();
  P.rec = L.add(sizeof(double) * kTriRec * nc);
  return P;
}

// ---------------------------------------------------------------------------
// ba_pnp_ransac / ba_pnp_hypotheses
// ---------------------------------------------------------------------------
inline void pnp_defaults(ba_pnp_options& o) {
  o.max_hypotheses = 1000; o.min_points = 7; o.min_inliers = 6; o.use_prior = 1; o.refine = 1; o.reserved = 0;
  o.seed = 0; o.threshold_px = 8.0;
}

// Everything the kernels index with or branch on, checked on the host: the
// batch, the options (returned with the defaults applied) and, with refine,
// the LM options.  lm: the resolved LM options, or null when they are not read.
inline ba_pnp_options check_pnp(const char* fn, const ba_pose_batch* b, const ba_pnp_options* popt, const ba_options* lm) {
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what}; };
  if (!b || b->n_problems < 0) throw invalid("bad batch");
  ba_pnp_options p;
  if (popt) p = *popt; else pnp_defaults(p);
  if (p.max_hypotheses < 1 || p.max_hypotheses > 65536)
    throw invalid("max_hypotheses " + std::to_string(p.max_hypotheses) + " outside 1 .. 65536");
  if (p.min_points < 0) throw invalid("min_points " + std::to_string(p.min_points) + " is negative");
  if (p.min_inliers < 0) throw invalid("min_inliers " + std::to_string(p.min_inliers) + " is negative");
  if (p.use_prior != 0 && p.use_prior != 1) throw invalid("unknown use_prior " + std::to_string(p.use_prior));
  if (p.refine != 0 && p.refine != 1) throw invalid("unknown refine " + std::to_string(p.refine));
  if (!(p.threshold_px > 0.0 && p.threshold_px <= 1.7976931348623157e308))
    throw invalid("threshold_px must be positive and finite");
  if (p.refine && lm) {
    if (lm->linear_solver != BA_DENSE_SCHUR) throw invalid("linear_solver must be BA_DENSE_SCHUR");
    if (lm->precision != BA_FP64) throw invalid("precision must be BA_FP64");
  }
  const int n = b->n_problems;
  if (n == 0) return p;
  if (!b->obs_offset || !b->K) throw invalid("null array");
  if (p.use_prior && !b->cams) throw invalid("use_prior is set but cams is null");
  check_offsets(fn, "obs_offset", b->obs_offset, n);
  if (b->obs_offset[n] > 0 && (!b->pts || !b->obs_uv)) throw invalid("null array");
  return p;
}

// Lanes per hypothesis of the scoring kernel: 8 while the batch, at one wave
// per 64 hypotheses, would occupy at most 64 waves (a single frame leaves the
// chip idle and is bound by the serial walk over its points), else 1.  The
// votes are integers, so the results do not depend on the choice.
inline int pnp_group(size_t N, int H) { return N * (((size_t)H + 63) / 64) <= 64 ? 8 : 1; }

// The staging buffer of the two entries.  ba_pnp_ransac (dbg_n == 0): the
// batch | cams_out, cam_ransac, LM summaries, result records, inlier mask |
// wave records, consensus mask, counts, dense offsets, compacted observations.
// ba_pnp_hypotheses (dbg_n > 0): the batch | the four inspection arrays.
struct PnpLayout {
  SectionLayout L{256};
  size_t off = 0, prior = 0, K = 0, X = 0, uv = 0;
  size_t cams_out = 0, cam_ransac = 0, summ = 0, res = 0, inlier = 0;
  size_t rec = 0, cmask = 0, cnt = 0, coff = 0, Xc = 0, uvc = 0;
  size_t dbg_sample = 0, dbg_nsol = 0, dbg_Rt = 0, dbg_count = 0;
};
inline PnpLayout pnp_layout(size_t N, size_t NO, int H, int G, size_t dbg_n) {
  PnpLayout P;
  SectionLayout& L = P.L;
  P.off = L.add(sizeof(int32_t) * (N + 1)); P.prior = L.add(sizeof(double) * 6 * N); P.K = L.add(sizeof(float) * 9 * N);
  P.X = L.add(sizeof(double) * 3 * NO); P.uv = L.add(sizeof(float) * 2 * NO);
  L.end_inputs();
  if (dbg_n > 0) {
    P.dbg_sample = L.add(sizeof(int32_t) * 3 * dbg_n); P.dbg_nsol = L.add(sizeof(int32_t) * dbg_n);
    P.dbg_Rt = L.add(sizeof(double) * 48 * dbg_n); P.dbg_count = L.add(sizeof(int32_t) * 4 * dbg_n);
    L.end_outputs();
    return P;
  }
  P.cams_out = L.add(sizeof(double) * 6 * N); P.cam_ransac = L.add(sizeof(double) * 6 * N);
  P.summ = L.add(sizeof(double) * 8 * N); P.res = L.add(sizeof(int32_t) * 4 * N); P.inlier = L.add(NO);
  L.end_outputs();
  const size_t hpw = 64 / (size_t)G, nw = ((size_t)H + hpw - 1) / hpw;
  P.rec = L.add(sizeof(double) * 16 * nw * N); P.cmask = L.add(NO); P.cnt = L.add(sizeof(int32_t) * N);
  P.coff = L.add(sizeof(int32_t) * (N + 1)); P.Xc = L.add(sizeof(double) * 3 * NO); P.uvc = L.add(sizeof(float) * 2 * NO);
  return P;
}

// ---------------------------------------------------------------------------
// ba_two_view_ransac / ba_two_view_hypotheses
// ---------------------------------------------------------------------------
inline void two_view_defaults(ba_two_view_options& o) {
  o.max_hypotheses = 1000; o.min_points = 8; o.min_inliers = 8; o.min_good = 101; o.model = BA_TV_AUTO; o.reserved = 0;
  o.seed = 0; o.threshold_px = 1.0; o.h_ratio = 0.4;
}

// Everything the kernels index with or branch on, checked on the host; the
// options are returned with the defaults applied.
inline ba_two_view_options check_two_view(const char* fn, const ba_two_view_batch* b, const ba_two_view_options* opt) {
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what}; };
  if (!b || b->n_pairs < 0) throw invalid("bad batch");
  ba_two_view_options p;
  if (opt) p = *opt; else two_view_defaults(p);
  if (p.max_hypotheses < 1 || p.max_hypotheses > 65536)
    throw invalid("max_hypotheses " + std::to_string(p.max_hypotheses) + " outside 1 .. 65536");
  if (p.min_points < 0) throw invalid("min_points " + std::to_string(p.min_points) + " is negative");
  if (p.min_inliers < 0) throw invalid("min_inliers " + std::to_string(p.min_inliers) + " is negative");
  if (p.min_good < 0) throw invalid("min_good " + std::to_string(p.min_good) + " is negative");
  if (p.model != BA_TV_AUTO && p.model != BA_TV_ESSENTIAL && p.model != BA_TV_HOMOGRAPHY)
    throw invalid("unknown model " + std::to_string(p.model));
  if (p.reserved != BA_TV_E_EIGHT_POINT && p.reserved != BA_TV_E_FIVE_POINT)
    throw invalid("unknown e_solver " + std::to_string(p.reserved));
  if (!(p.threshold_px > 0.0 && p.threshold_px <= 1.7976931348623157e308))
    throw invalid("threshold_px must be positive and finite");
  if (!(p.h_ratio >= 0.0 && p.h_ratio <= 1.0)) throw invalid("h_ratio must lie in [0, 1]");
  const int n = b->n_pairs;
  if (n == 0) return p;
  if (!b->match_offset || !b->K1) throw invalid("null array");
  check_offsets(fn, "match_offset", b->match_offset, n, "pair");
  if (b->match_offset[n] > 0 && (!b->uv1 || !b->uv2)) throw invalid("null array");
  return p;
}

// The staging buffer of the entries.  ba_two_view_ransac (dbg_n == 0):
// offsets, K1, K2, matches as (u1, v1, u2, v2) | result records, inlier mask |
// models, validity, wave records and, in five-point mode only (e5), the
// solutions (720 B per hypothesis), their counts per hypothesis and the wave
// records of their vote.  ba_two_view_hypotheses (dbg_n > 0): the batch |
// samples, models, validity, counts of the dbg_n hypotheses;
// ba_two_view_hypotheses_e5 (dbg_n > 0, e5): the batch | samples, solution
// counts, solutions, votes.
struct TwoViewLayout {
  SectionLayout L{256};
  size_t off = 0, K1 = 0, K2 = 0, m = 0;
  size_t res = 0, inlier = 0;
  size_t models = 0, valid = 0, rec = 0;
  size_t models5 = 0, nsol5 = 0, rec5 = 0;
  size_t dbg_sample = 0, dbg_count = 0, dbg_count5 = 0;
};
inline TwoViewLayout two_view_layout(size_t N, size_t NM, int H, int G, size_t dbg_n, bool e5 = false, int G5 = 1) {
  TwoViewLayout P;
  SectionLayout& L = P.L;
  P.off = L.add(sizeof(int32_t) * (N + 1)); P.K1 = L.add(sizeof(float) * 9 * N); P.K2 = L.add(sizeof(float) * 9 * N);
  P.m = L.add(sizeof(float) * 4 * NM);
  L.end_inputs();
  if (dbg_n > 0 && e5) {
    P.dbg_sample = L.add(sizeof(int32_t) * 8 * dbg_n); P.nsol5 = L.add(sizeof(int32_t) * dbg_n);
    P.models5 = L.add(sizeof(double) * 90 * dbg_n); P.dbg_count5 = L.add(sizeof(int32_t) * 10 * dbg_n);
    L.end_outputs();
    return P;
  }
  if (dbg_n > 0) {
    P.dbg_sample = L.add(sizeof(int32_t) * 8 * dbg_n); P.models = L.add(sizeof(double) * 18 * dbg_n);
    P.valid = L.add(sizeof(int32_t) * 2 * dbg_n); P.dbg_count = L.add(sizeof(int32_t) * 2 * dbg_n);
    L.end_outputs();
    return P;
  }
  P.res = L.add(sizeof(double) * 40 * N); P.inlier = L.add(NM);
  L.end_outputs();
  const size_t hpw = 64 / (size_t)G, nw = ((size_t)H + hpw - 1) / hpw;
  P.models = L.add(sizeof(double) * 18 * (size_t)H * N); P.valid = L.add(sizeof(int32_t) * 2 * (size_t)H * N);
  P.rec = L.add(sizeof(uint64_t) * 2 * nw * N);
  if (e5) {
    const size_t hpw5 = 64 / (size_t)G5, nw5 = (10 * (size_t)H + hpw5 - 1) / hpw5;
    P.models5 = L.add(sizeof(double) * 90 * (size_t)H * N); P.nsol5 = L.add(sizeof(int32_t) * (size_t)H * N);
    P.rec5 = L.add(sizeof(uint64_t) * nw5 * N);
  }
  return P;
}
// The matches of a batch as the kernels read them: (u1, v1, u2, v2) per match
inline void two_view_pack_matches(const ba_two_view_batch* b, size_t NM, float* dst) {
  for (size_t k = 0; k < NM; ++k) {
    dst[4 * k] = b->uv1[2 * k]; dst[4 * k + 1] = b->uv1[2 * k + 1];
    dst[4 * k + 2] = b->uv2[2 * k]; dst[4 * k + 3] = b->uv2[2 * k + 1];
  }
}

// ---------------------------------------------------------------------------
// ba_match_descriptors / ba_match_knn
// ---------------------------------------------------------------------------
inline void match_defaults(ba_match_options& o) {
  o.ratio = 0.7f; o.unique = 1; o.max_distance = std::numeric_limits<float>::infinity(); o.reserved = 0;
}

constexpr int kMatchQTile = 128;        // query rows per workgroup of the 2-NN kernel
constexpr int kMatchTTile = 64;         // train rows per staged tile
constexpr int kMatchMaxRows = 65535 * kMatchQTile;   // a grid dimension holds a set's query tiles

// One pair as the kernels read it
struct MatchPair {
  int q0, nq;      // the query set: first row in desc, rows
  int t0, nt;      // the train set
  int qoff;        // first dense 2-NN record (sum of nq of the pairs before)
  int toff;        // first per-train slot (sum of nt of the pairs before)
  int moff;        // first match record (sum of the capacities of the pairs before)
  int cap;         // match capacity: min(nq, nt) with unique, else nq
};

// Everything the kernels index with or branch on, checked on the host; the
// options are returned with the defaults applied.
inline ba_match_options check_match(const char* fn, const ba_match_batch* b, const ba_match_options* opt) {
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what}; };
  if (!b || b->n_sets < 0 || b->n_pairs < 0 || b->n_ref < 0) throw invalid("bad batch");
  if (b->dim != 64 && b->dim != 128) throw invalid("dim " + std::to_string(b->dim) + " is neither 64 nor 128");
  ba_match_options p;
  if (opt) p = *opt; else match_defaults(p);
  if (!(p.ratio >= 0.0f && p.ratio <= std::numeric_limits<float>::max())) throw invalid("ratio must be non-negative and finite");
  if (!(p.max_distance >= 0.0f)) throw invalid("max_distance must be non-negative");
  if (p.unique != 0 && p.unique != 1) throw invalid("unknown unique " + std::to_string(p.unique));
  if (p.reserved != 0) throw invalid("reserved must be 0");
  if (b->n_sets > 0 && !b->set_offset) throw invalid("null array");
  if (b->n_sets > 0) check_offsets(fn, "set_offset", b->set_offset, b->n_sets, "set");
  const int rows = b->n_sets > 0 ? b->set_offset[b->n_sets] : 0;
  for (int s = 0; s < b->n_sets; ++s)
    if (b->set_offset[s + 1] - b->set_offset[s] > kMatchMaxRows)
      throw invalid("set " + std::to_string(s) + " has more than " + std::to_string(kMatchMaxRows) + " rows");
  if (rows > 0 && !b->desc) throw invalid("null array");
  if (b->n_pairs > 0 && (!b->pair_query || !b->pair_train)) throw invalid("null array");
  for (int i = 0; i < b->n_pairs; ++i)
    if (b->pair_query[i] < 0 || b->pair_query[i] >= b->n_sets || b->pair_train[i] < 0 || b->pair_train[i] >= b->n_sets)
      throw invalid("pair " + std::to_string(i) + " names a set out of range");
  if (b->row_ref)
    for (int r = 0; r < rows; ++r) {
      if (b->row_ref[r] < -1 || b->row_ref[r] >= b->n_ref)
        throw invalid("row_ref[" + std::to_string(r) + "] out of range");
      if (b->row_ref[r] >= 0 && !b->ref_desc) throw invalid("row_ref names a reference but ref_desc is null");
    }
  return p;
}

// The pair table, the totals and the split of the train sets into chunks.
// Chunks: one pair of 2000 queries is 16 workgroups on 256 compute units, so
// the train rows are dealt to `chunks` workgroups per query tile (chunk_rows
// each, a multiple of the staged tile and at least two tiles) until the batch
// offers about two workgroups per unit; the partial top-2 lists merge by key,
// so the result does not depend on the split.
struct MatchPlan {
  std::vector<MatchPair> pair;
  size_t NQ = 0, NT = 0, NM = 0;      // dense records, train slots, match capacity
  int max_nq = 0, max_nt = 0;
  int chunks = 1, chunk_rows = kMatchTTile;
};
inline MatchPlan match_plan(const char* fn, const ba_match_batch* b, int unique, int first_pair, int n_pairs) {
  MatchPlan M;
  M.pair.resize((size_t)n_pairs);
  size_t tiles = 0;
  for (int i = 0; i < n_pairs; ++i) {
    MatchPair& P = M.pair[(size_t)i];
    const int sq = b->pair_query[first_pair + i], st = b->pair_train[first_pair + i];
    P.q0 = b->set_offset[sq]; P.nq = b->set_offset[sq + 1] - P.q0;
    P.t0 = b->set_offset[st]; P.nt = b->set_offset[st + 1] - P.t0;
    P.cap = unique ? std::min(P.nq, P.nt) : P.nq;
    P.qoff = (int)M.NQ; P.toff = (int)M.NT; P.moff = (int)M.NM;
    M.NQ += (size_t)P.nq; M.NT += (size_t)P.nt; M.NM += (size_t)P.cap;
    M.max_nq = std::max(M.max_nq, P.nq); M.max_nt = std::max(M.max_nt, P.nt);
    tiles += ((size_t)P.nq + kMatchQTile - 1) / kMatchQTile;
  }
  if (M.NQ > 0x7fffffffull || M.NT > 0x7fffffffull)
    throw BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + "the pairs hold more than 2^31 - 1 query or train rows"};
  if (tiles > 0 && M.max_nt > 0) {
    const size_t want = (512 + tiles - 1) / tiles;
    const size_t most = ((size_t)M.max_nt + 2 * kMatchTTile - 1) / (2 * kMatchTTile);
    M.chunks = (int)std::max<size_t>(1, std::min(want, most));
    const int per = (M.max_nt + M.chunks - 1) / M.chunks;
    M.chunk_rows = (per + kMatchTTile - 1) / kMatchTTile * kMatchTTile;
    M.chunks = (M.max_nt + M.chunk_rows - 1) / M.chunk_rows;
  }
  return M;
}

// The staging buffer.  ba_match_descriptors (knn == false): the pair table,
// row_ref, reference descriptors, descriptors | counts, match records | norms,
// partial top-2 lists, dense records, survivor flags, per-train winners,
// per-train counts.  ba_match_knn (knn == true): the same inputs | the dense
// records | norms, partial lists.
struct MatchLayout {
  SectionLayout L{256};
  size_t pair = 0, desc = 0, row_ref = 0, ref = 0;
  size_t cnt = 0, matches = 0;
  size_t norms = 0, part = 0, knn = 0, surv = 0, win = 0, hist = 0;
};
inline MatchLayout match_layout(const MatchPlan& M, size_t rows, size_t n_ref, int dim, bool have_ref, bool knn) {
  MatchLayout P;
  SectionLayout& L = P.L;
  const size_t N = M.pair.size();
  P.pair = L.add(sizeof(MatchPair) * N);
  P.row_ref = L.add(have_ref ? sizeof(int32_t) * rows : 0); P.ref = L.add(have_ref ? sizeof(float) * n_ref * (size_t)dim : 0);
  P.desc = L.add(sizeof(float) * rows * (size_t)dim);   // the last input: uploaded from the caller's array
  L.end_inputs();
  if (knn) {
    P.knn = L.add(sizeof(ba_match_neighbors) * M.NQ);
    L.end_outputs();
  } else {
    P.cnt = L.add(sizeof(int32_t) * N); P.matches = L.add(sizeof(ba_match) * M.NM);
    L.end_outputs();
    P.knn = L.add(sizeof(ba_match_neighbors) * M.NQ); P.surv = L.add(M.NQ);
    P.win = L.add(sizeof(uint64_t) * M.NT); P.hist = L.add(sizeof(int32_t) * M.NT);
  }
  P.norms = L.add(sizeof(float) * (rows + (have_ref ? n_ref : 0)));
  P.part = L.add(sizeof(uint64_t) * 2 * M.NQ * (size_t)M.chunks);
  return P;
}

// ---------------------------------------------------------------------------
// ba_map_points_update / ba_map_points_distances / ba_associate
// ---------------------------------------------------------------------------
inline void map_points_defaults(ba_map_point_options& o) {
  o.median_rule = BA_MP_MEDIAN_REFERENCE; o.reserved = 0; o.max_scale = 3.5831808f; o.reserved_f = 0.0f;
}
inline void assoc_defaults(ba_assoc_options& o) {
  o.chi2 = 5.991f; o.min_cos = 0.5f; o.max_desc_dist = 0.2f; o.fuse_min_cos = 0.0f; o.fuse_max_desc_dist = 0.3f;
  o.reserved = 0;
}

// Everything the kernels index with or branch on, checked on the host; the
// options are returned with the defaults applied.
inline ba_map_point_options check_map_points(const char* fn, const ba_map_point_batch* b, const ba_map_point_options* opt) {
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what}; };
  if (!b || b->n_cams < 0 || b->n_pts < 0 || b->n_rows < 0) throw invalid("bad batch");
  if (b->dim != 64 && b->dim != 128) throw invalid("dim " + std::to_string(b->dim) + " is neither 64 nor 128");
  ba_map_point_options p;
  if (opt) p = *opt; else map_points_defaults(p);
  if (p.median_rule != BA_MP_MEDIAN_REFERENCE && p.median_rule != BA_MP_MEDIAN_FLOAT)
    throw invalid("unknown median_rule " + std::to_string(p.median_rule));
  if (!(p.max_scale > 0.0f && p.max_scale <= std::numeric_limits<float>::max()))
    throw invalid("max_scale must be positive and finite");
  if (p.reserved != 0 || p.reserved_f != 0.0f) throw invalid("reserved must be 0");
  const int np = b->n_pts;
  if (np == 0) return p;
  if (!b->obs_offset || !b->pts) throw invalid("null array");
  check_offsets(fn, "obs_offset", b->obs_offset, np, "point");
  const int no = b->obs_offset[np];
  if (no > 0 && (!b->obs_cam || !b->obs_row || !b->cam_center || !b->desc)) throw invalid("null array");
  for (int q = 0; q < np; ++q) {
    const int n = b->obs_offset[q + 1] - b->obs_offset[q];
    if (n > BA_MP_MAX_TRACK)
      throw invalid("point " + std::to_string(q) + " has a track of " + std::to_string(n) + " observations, more than " +
                    std::to_string(BA_MP_MAX_TRACK));
    if (b->ref_obs && n > 0 && (b->ref_obs[q] < 0 || b->ref_obs[q] >= n))
      throw invalid("ref_obs[" + std::to_string(q) + "] out of range");
  }
  for (int o = 0; o < no; ++o) {
    if (b->obs_cam[o] < 0 || b->obs_cam[o] >= b->n_cams) throw invalid("obs_cam[" + std::to_string(o) + "] out of range");
    if (b->obs_row[o] < 0 || b->obs_row[o] >= b->n_rows) throw invalid("obs_row[" + std::to_string(o) + "] out of range");
  }
  return p;
}

// Points sorted into tiers by track length, so that a point takes the lanes
// and the LDS its track needs: up to kMpShort observations a group of 16
// lanes, up to kMpWave a wave, longer tracks a workgroup.  order lists the
// points tier by tier, each tier in batch order; the kernels write a point's
// record at its own index, and a point's bits do not depend on its tier.
constexpr int kMpShort = 16, kMpWave = 64;
struct MapPointsPlan {
  std::vector<int32_t> order;
  int first[3] = {0, 0, 0}, count[3] = {0, 0, 0};
};
inline int map_points_tier(int n) { return n <= kMpShort ? 0 : n <= kMpWave ? 1 : 2; }
inline MapPointsPlan map_points_plan(const ba_map_point_batch* b, int first_pt, int n_pts) {
  MapPointsPlan M;
  M.order.resize((size_t)n_pts);
  for (int i = 0; i < n_pts; ++i) ++M.count[map_points_tier(b->obs_offset[first_pt + i + 1] - b->obs_offset[first_pt + i])];
  M.first[1] = M.count[0]; M.first[2] = M.count[0] + M.count[1];
  int next[3] = {M.first[0], M.first[1], M.first[2]};
  for (int i = 0; i < n_pts; ++i)
    M.order[(size_t)next[map_points_tier(b->obs_offset[first_pt + i + 1] - b->obs_offset[first_pt + i])]++] = first_pt + i;
  return M;
}

// The staging buffer of ba_map_points_update (dbg_n == 0): the tables, then
// the descriptors | the records, the chosen descriptors.  ba_map_points_distances
// (dbg_n = the point's track length): the same inputs | one record, D, m.
struct MapPointsLayout {
  SectionLayout L{256};
  size_t center = 0, pts = 0, off = 0, cam = 0, row = 0, scale = 0, ref = 0, order = 0, desc = 0;
  size_t out = 0, desc_out = 0, dbg_D = 0, dbg_m = 0;
};
inline MapPointsLayout map_points_layout(const ba_map_point_batch* b, size_t n_order, bool want_desc, size_t dbg_n) {
  MapPointsLayout P;
  SectionLayout& L = P.L;
  const size_t np = (size_t)b->n_pts, no = np ? (size_t)b->obs_offset[np] : 0, dim = (size_t)b->dim;
  P.center = L.add(sizeof(float) * 3 * (size_t)b->n_cams); P.pts = L.add(sizeof(float) * 3 * np);
  P.off = L.add(sizeof(int32_t) * (np + 1)); P.cam = L.add(sizeof(int32_t) * no); P.row = L.add(sizeof(int32_t) * no);
  P.scale = L.add(b->obs_scale ? sizeof(float) * no : 0); P.ref = L.add(b->ref_obs ? sizeof(int32_t) * np : 0);
  P.order = L.add(sizeof(int32_t) * n_order);
  P.desc = L.add(sizeof(float) * (size_t)b->n_rows * dim);   // the last input: uploaded from the caller's array
  L.end_inputs();
  if (dbg_n > 0) {
    P.out = L.add(sizeof(ba_map_point)); P.dbg_D = L.add(sizeof(float) * dbg_n * dbg_n); P.dbg_m = L.add(sizeof(float) * dbg_n);
  } else {
    P.out = L.add(sizeof(ba_map_point) * np); P.desc_out = L.add(want_desc ? sizeof(float) * np * dim : 0);
  }
  L.end_outputs();
  return P;
}

inline ba_assoc_options check_assoc(const char* fn, const ba_assoc_batch* b, const ba_assoc_options* opt) {
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what}; };
  if (!b || b->n_cams < 0 || b->n_pts < 0 || b->n_rows < 0 || b->n_items < 0 || b->n_fuse < 0) throw invalid("bad batch");
  if (b->dim != 64 && b->dim != 128) throw invalid("dim " + std::to_string(b->dim) + " is neither 64 nor 128");
  ba_assoc_options p;
  if (opt) p = *opt; else assoc_defaults(p);
  if (p.reserved != 0) throw invalid("reserved must be 0");
  if (b->n_items > 0 && (!b->extr || !b->cam_center || !b->K || !b->image_size || !b->pts || !b->pt_view_dir ||
                         !b->pt_dist || !b->pt_desc || !b->desc || !b->item_cam || !b->item_pt || !b->item_uv ||
                         !b->item_row))
    throw invalid("null array");
  if (b->n_fuse > 0 && (!b->pt_view_dir || !b->pt_desc || !b->fuse_pairs)) throw invalid("null array");
  for (int i = 0; i < b->n_items; ++i) {
    const std::string at = "[" + std::to_string(i) + "] out of range";
    if (b->item_cam[i] < 0 || b->item_cam[i] >= b->n_cams) throw invalid("item_cam" + at);
    if (b->item_pt[i] < 0 || b->item_pt[i] >= b->n_pts) throw invalid("item_pt" + at);
    if (b->item_row[i] < 0 || b->item_row[i] >= b->n_rows) throw invalid("item_row" + at);
    if (b->item_cur_row && (b->item_cur_row[i] < -1 || b->item_cur_row[i] >= b->n_rows)) throw invalid("item_cur_row" + at);
  }
  for (int i = 0; i < 2 * b->n_fuse; ++i)
    if (b->fuse_pairs[i] < 0 || b->fuse_pairs[i] >= b->n_pts)
      throw invalid("fuse_pairs[" + std::to_string(i) + "] out of range (pair " + std::to_string(i / 2) + ")");
  return p;
}

// The staging buffer of ba_associate: cameras, points, items, fuse pairs, the
// two descriptor tables | item results, fuse results.
struct AssocLayout {
  SectionLayout L{256};
  size_t extr = 0, center = 0, K = 0, size = 0, pts = 0, dir = 0, dist = 0, cam = 0, pt = 0, uv = 0, scale = 0, row = 0,
         cur = 0, fuse = 0, pt_desc = 0, desc = 0;
  size_t items = 0, fused = 0;
};
inline AssocLayout assoc_layout(const ba_assoc_batch* b) {
  AssocLayout P;
  SectionLayout& L = P.L;
  const size_t nc = (size_t)b->n_cams, np = (size_t)b->n_pts, ni = (size_t)b->n_items, nf = (size_t)b->n_fuse, dim = (size_t)b->dim;
  P.extr = L.add(sizeof(float) * 16 * nc); P.center = L.add(sizeof(float) * 3 * nc); P.K = L.add(sizeof(float) * 9 * nc);
  P.size = L.add(sizeof(int32_t) * 2 * nc); P.pts = L.add(sizeof(float) * 3 * np); P.dir = L.add(sizeof(float) * 3 * np);
  P.dist = L.add(sizeof(float) * 2 * np); P.cam = L.add(sizeof(int32_t) * ni); P.pt = L.add(sizeof(int32_t) * ni);
  P.uv = L.add(sizeof(float) * 2 * ni); P.scale = L.add(b->item_scale ? sizeof(float) * ni : 0);
  P.row = L.add(sizeof(int32_t) * ni); P.cur = L.add(b->item_cur_row ? sizeof(int32_t) * ni : 0);
  P.fuse = L.add(sizeof(int32_t) * 2 * nf);
  P.pt_desc = L.add(sizeof(float) * np * dim); P.desc = L.add(sizeof(float) * (size_t)b->n_rows * dim);
  L.end_inputs();
  P.items = L.add(sizeof(ba_assoc_result) * ni); P.fused = L.add(sizeof(ba_fuse_result) * nf);
  L.end_outputs();
  return P;
}

// ---------------------------------------------------------------------------
// ba_map_graph / ba_map_graph_weights
// ---------------------------------------------------------------------------
inline void map_graph_defaults(ba_graph_options& o) {
  o.th = 10; o.n_best = 10; o.order = BA_GRAPH_WEAKEST_FIRST; o.build_windows = 1; o.current_frame_id = 0;
  o.debug_tile_frames = 0; o.debug_chunk_queries = 0; o.reserved = 0; o.redundant_fraction = 0.95;
}

// Everything the kernels index with or branch on, checked on the host; the
// options are returned with the defaults applied.
inline ba_graph_options check_map_table(const char* fn, const ba_map_table* t, const int32_t* query, int n_query,
                                        const ba_graph_options* opt, bool want_status) {
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what}; };
  if (!t || t->n_frames < 0 || t->n_pts < 0 || t->n_obs < 0 || n_query < 0) throw invalid("bad table");
  if (t->reserved != 0) throw invalid("reserved must be 0");
  ba_graph_options p;
  if (opt) p = *opt; else map_graph_defaults(p);
  if (p.n_best < 0 || p.n_best > BA_WINDOW_MAX_CAMS - 1)
    throw invalid("n_best " + std::to_string(p.n_best) + " outside 0 .. " + std::to_string(BA_WINDOW_MAX_CAMS - 1));
  if (p.order != BA_GRAPH_WEAKEST_FIRST && p.order != BA_GRAPH_STRONGEST_FIRST)
    throw invalid("unknown order " + std::to_string(p.order));
  if (p.th < 0) throw invalid("th " + std::to_string(p.th) + " is negative");
  if (!(p.redundant_fraction >= -std::numeric_limits<double>::max() && p.redundant_fraction <= std::numeric_limits<double>::max()))
    throw invalid("redundant_fraction must be finite");
  if (p.debug_tile_frames < 0 || p.debug_chunk_queries < 0) throw invalid("a debug field is negative");
  if (p.reserved != 0) throw invalid("reserved must be 0");
  if (want_status && t->n_pts > 0 && !t->pt_ref_frame) throw invalid("pt_status needs pt_ref_frame");
  if (t->n_frames > 0 && !t->frame_id) throw invalid("null array frame_id");
  if (!t->obs_offset) throw invalid("null array obs_offset");
  check_offsets(fn, "obs_offset", t->obs_offset, t->n_pts, "point");
  if (t->obs_offset[t->n_pts] != t->n_obs)
    throw invalid("obs_offset[n_pts] is " + std::to_string(t->obs_offset[t->n_pts]) + ", not n_obs " + std::to_string(t->n_obs));
  if (t->n_obs > 0 && !t->obs_frame) throw invalid("null array obs_frame");
  for (int o = 0; o < t->n_obs; ++o)
    if (t->obs_frame[o] < 0 || t->obs_frame[o] >= t->n_frames) throw invalid("obs_frame[" + std::to_string(o) + "] out of range");
  if (t->pt_ref_frame)
    for (int q = 0; q < t->n_pts; ++q)
      if (t->pt_ref_frame[q] < 0 || t->pt_ref_frame[q] >= t->n_frames)
        throw invalid("pt_ref_frame[" + std::to_string(q) + "] out of range");
  if (n_query > 0 && !query) throw invalid("null array query");
  for (int i = 0; i < n_query; ++i)
    if (query[i] < 0 || query[i] >= t->n_frames) throw invalid("query[" + std::to_string(i) + "] out of range");
  return p;
}

// The frame-sorted view of the table: frame f owns perm[frame_off[f] ..
// frame_off[f+1]), its observations in ascending o (count, scan, stable
// scatter), and obs_pt[o] is the point of observation o.
struct MapGraphPlan {
  std::vector<int32_t> frame_off, perm, obs_pt;
};
inline MapGraphPlan map_graph_plan(const ba_map_table* t) {
  MapGraphPlan M;
  const size_t nf = (size_t)t->n_frames, no = (size_t)t->n_obs;
  M.frame_off.assign(nf + 1, 0); M.perm.resize(no); M.obs_pt.resize(no);
  for (size_t o = 0; o < no; ++o) ++M.frame_off[(size_t)t->obs_frame[o] + 1];
  for (size_t f = 0; f < nf; ++f) M.frame_off[f + 1] += M.frame_off[f];
  std::vector<int32_t> next(M.frame_off.begin(), M.frame_off.end() - 1);
  for (int p = 0; p < t->n_pts; ++p)
    for (int o = t->obs_offset[p]; o < t->obs_offset[p + 1]; ++o) {
      M.obs_pt[(size_t)o] = p;
      M.perm[(size_t)next[(size_t)t->obs_frame[o]]++] = o;
    }
  return M;
}

inline int map_graph_tile(const ba_graph_options& p, int n_frames) {
  const int T = p.debug_tile_frames > 0 ? p.debug_tile_frames : kMgTileMax;
  return std::max(1, std::min(std::min(T, kMgTileMax), std::max(n_frames, 1)));
}
inline size_t map_graph_words(int n) { return ((size_t)n + 31) / 32; }
// Device scratch of one query: the W row, the sorted list (frame, weight), the
// best frames, the local / fixed frame bitmaps with the fixed prefix counts,
// and the point bitmap
inline size_t map_graph_query_bytes(const ba_map_table* t, bool windows) {
  const size_t nf = (size_t)t->n_frames;
  return 4 * (3 * nf + BA_WINDOW_MAX_CAMS + 3 * map_graph_words(t->n_frames) + (windows ? map_graph_words(t->n_pts) : 0)) + 64;
}
inline int map_graph_chunk(const ba_graph_options& p, const ba_map_table* t, int n_query) {
  if (p.debug_chunk_queries > 0) return std::min(p.debug_chunk_queries, std::max(n_query, 1));
  const size_t fit = kMgChunkBudget / map_graph_query_bytes(t, p.build_windows != 0);
  return (int)std::max<size_t>(1, std::min<size_t>(fit, (size_t)std::max(n_query, 1)));
}

// The staging buffer: the table (from the caller's arrays), its frame-sorted
// view and the queries | the records, the point status | the scratch of `chunk`
// queries (map_graph_query_bytes lists it) and their list offsets.
struct MapGraphLayout {
  SectionLayout L{256};
  size_t frame_id = 0, is_key = 0, pt_invalid = 0, pt_ref = 0, off = 0, frame = 0, octave = 0, outlier = 0, obs_pt = 0,
         perm = 0, frame_off = 0, query = 0;
  size_t rec = 0, status = 0;
  size_t W = 0, lst_f = 0, lst_w = 0, best = 0, loc = 0, fix = 0, pre = 0, ptb = 0, offs = 0;
};
static inline MapGraphLayout map_graph_layout(const ba_map_table* t, const ba_graph_options& p, int n_query, int chunk, bool want_status) {
  MapGraphLayout P;
  SectionLayout& L = P.L;
  const size_t nf = (size_t)t->n_frames, np = (size_t)t->n_pts, no = (size_t)t->n_obs, nq = (size_t)n_query,
               fw = map_graph_words(t->n_frames), pw = p.build_windows ? map_graph_words(t->n_pts) : 0, nc = (size_t)chunk;
  P.frame_id = L.add(4 * nf); P.is_key = L.add(t->frame_is_key ? nf : 0); P.pt_invalid = L.add(t->pt_invalid ? np : 0);
  P.pt_ref = L.add(want_status ? 4 * np : 0); P.off = L.add(4 * (np + 1)); P.frame = L.add(4 * no);
  P.octave = L.add(t->obs_octave ? 4 * no : 0); P.outlier = L.add(t->obs_outlier ? no : 0); P.obs_pt = L.add(4 * no);
  P.perm = L.add(4 * no); P.frame_off = L.add(4 * (nf + 1)); P.query = L.add(4 * nq);
  L.end_inputs();
  P.rec = L.add(sizeof(ba_graph_frame) * nq); P.status = L.add(want_status ? np : 0);
  L.end_outputs();
  P.W = L.add(4 * nc * nf); P.lst_f = L.add(4 * nc * nf); P.lst_w = L.add(4 * nc * nf);
  P.best = L.add(4 * nc * BA_WINDOW_MAX_CAMS); P.loc = L.add(4 * nc * fw); P.fix = L.add(4 * nc * fw);
  P.pre = L.add(4 * nc * fw); P.ptb = L.add(4 * nc * pw); P.offs = L.add(sizeof(long long) * 4 * nc);
  return P;
}

// The plain restatement of ba_map_graph, query by query, on one thread: what
// the kernels of ba_map_graph.hip compute (tests/cpp/map_graph_host.cpp runs it
// under ASan + UBSan; tools/map_graph_bench.py times it).
struct MapGraphHost {
  std::vector<ba_graph_frame> rec;
  std::vector<int32_t> nbr_frame, nbr_weight, win_cam, win_pt, win_obs, win_obs_cam, win_obs_pt;
  std::vector<uint8_t> win_cam_fixed, pt_status;
};
inline void map_graph_host_weights(const ba_map_table* t, const MapGraphPlan& M, int q, std::vector<int32_t>& W) {
  W.assign((size_t)t->n_frames, 0);
  for (int i = M.frame_off[(size_t)q]; i < M.frame_off[(size_t)q + 1]; ++i) {
    const int o = M.perm[(size_t)i];
    if (t->obs_outlier && t->obs_outlier[o]) continue;
    const int p = M.obs_pt[(size_t)o];
    for (int k = t->obs_offset[p]; k < t->obs_offset[p + 1]; ++k)
      if (t->obs_frame[k] != q) ++W[(size_t)t->obs_frame[k]];
  }
}
inline MapGraphHost map_graph_host(const ba_map_table* t, const MapGraphPlan& M, const int32_t* query, int n_query,
                                   const ba_graph_options& p, bool want_status) {
  MapGraphHost R;
  const int nf = t->n_frames;
  auto is_key = [&](int g) { return !t->frame_is_key || t->frame_is_key[g] != 0; };
  auto invalid = [&](int pt) { return t->pt_invalid && t->pt_invalid[pt] != 0; };
  auto outlier = [&](int o) { return t->obs_outlier && t->obs_outlier[o] != 0; };
  auto octave = [&](int o) { return t->obs_octave ? t->obs_octave[o] : 0; };
  std::vector<int32_t> W;
  std::vector<uint8_t> local((size_t)nf), fixed((size_t)nf), pt_local((size_t)t->n_pts);
  std::vector<int32_t> cam_of((size_t)nf), pt_rank((size_t)t->n_pts);
  for (int qi = 0; qi < n_query; ++qi) {
    const int q = query[qi];
    ba_graph_frame r{};
    map_graph_host_weights(t, M, q, W);
    std::vector<std::pair<uint64_t, int32_t>> list;
    uint64_t fb = 0;
    for (int g = 0; g < nf; ++g) {
      r.max_weight = std::max(r.max_weight, W[(size_t)g]);
      if (W[(size_t)g] > 0) fb = std::max(fb, mg_fallback_key(W[(size_t)g], g));
      if (W[(size_t)g] > p.th && is_key(g)) list.push_back({mg_list_key(W[(size_t)g], g), g});
    }
    r.status = BA_GRAPH_OK;
    if (list.empty()) {
      if (r.max_weight > 0) {
        const int32_t g = (int32_t)(0xffffffffu - (uint32_t)fb);
        list.push_back({mg_list_key(W[(size_t)g], g), g});
        r.status = BA_GRAPH_FALLBACK;
      } else {
        r.status = BA_GRAPH_ISOLATED;
      }
    }
    std::sort(list.begin(), list.end());
    r.degree = (int32_t)list.size();
    for (auto& e : list) { R.nbr_frame.push_back(e.second); R.nbr_weight.push_back(W[(size_t)e.second]); }
    std::vector<int32_t> best;
    for (auto& e : list) best.push_back(e.second);
    if (p.order == BA_GRAPH_STRONGEST_FIRST)
      std::sort(best.begin(), best.end(), [&](int32_t a, int32_t b) { return mg_stronger(W[(size_t)a], a, W[(size_t)b], b); });
    best.resize((size_t)std::min<int>(p.n_best, r.degree));
    // the vote
    for (int i = M.frame_off[(size_t)q]; i < M.frame_off[(size_t)q + 1]; ++i) {
      const int o = M.perm[(size_t)i], pt = M.obs_pt[(size_t)o];
      if (invalid(pt)) continue;
      ++r.n_map;
      if (t->obs_offset[pt + 1] - t->obs_offset[pt] <= kMgMinTrack) continue;
      int views = 0;
      for (int k = t->obs_offset[pt]; k < t->obs_offset[pt + 1]; ++k)
        views += t->obs_frame[k] != q && mg_view_counts(octave(k), octave(o)) ? 1 : 0;
      r.n_redundant += views >= kMgMinViews ? 1 : 0;
    }
    r.cull = mg_cull(t->frame_id[q], r.n_map, r.n_redundant, p.redundant_fraction);
    if (p.build_windows) {
      r.n_local = (int32_t)best.size() + 1;
      std::vector<int32_t> cams(best);
      cams.push_back(q);
      std::fill(local.begin(), local.end(), 0); std::fill(fixed.begin(), fixed.end(), 0);
      std::fill(pt_local.begin(), pt_local.end(), 0);
      for (size_t c = 0; c < cams.size(); ++c) { local[(size_t)cams[c]] = 1; cam_of[(size_t)cams[c]] = (int32_t)c; }
      for (int32_t f : cams)
        for (int i = M.frame_off[(size_t)f]; i < M.frame_off[(size_t)f + 1]; ++i) {
          const int o = M.perm[(size_t)i];
          if (!outlier(o) && !invalid(M.obs_pt[(size_t)o])) pt_local[(size_t)M.obs_pt[(size_t)o]] = 1;
        }
      for (int pt = 0; pt < t->n_pts; ++pt) {
        if (!pt_local[(size_t)pt]) continue;
        pt_rank[(size_t)pt] = r.n_win_pts++;
        R.win_pt.push_back(pt);
        for (int k = t->obs_offset[pt]; k < t->obs_offset[pt + 1]; ++k)
          if (!outlier(k) && !local[(size_t)t->obs_frame[k]] && is_key(t->obs_frame[k])) fixed[(size_t)t->obs_frame[k]] = 1;
      }
      for (int g = 0; g < nf; ++g)
        if (fixed[(size_t)g]) { cam_of[(size_t)g] = r.n_local + r.n_fixed++; cams.push_back(g); }
      for (size_t c = 0; c < cams.size(); ++c) {
        R.win_cam.push_back(cams[c]);
        R.win_cam_fixed.push_back((int)c >= r.n_local || t->frame_id[cams[c]] == 0 ? 1 : 0);
      }
      for (int pt = 0; pt < t->n_pts; ++pt) {
        if (!pt_local[(size_t)pt]) continue;
        for (int k = t->obs_offset[pt]; k < t->obs_offset[pt + 1]; ++k) {
          const int g = t->obs_frame[k];
          if (outlier(k) || !(local[(size_t)g] || fixed[(size_t)g])) continue;
          ++r.n_win_obs;
          R.win_obs.push_back(k); R.win_obs_cam.push_back(cam_of[(size_t)g]); R.win_obs_pt.push_back(pt_rank[(size_t)pt]);
        }
      }
    }
    R.rec.push_back(r);
  }
  if (want_status) {
    R.pt_status.resize((size_t)t->n_pts);
    for (int pt = 0; pt < t->n_pts; ++pt)
      R.pt_status[(size_t)pt] = mg_point_status(invalid(pt), (int64_t)p.current_frame_id - t->frame_id[t->pt_ref_frame[pt]],
                                                t->obs_offset[pt + 1] - t->obs_offset[pt]);
  }
  return R;
}

// ---------------------------------------------------------------------------
// ba_icp / ba_icp_nn
// ---------------------------------------------------------------------------
inline void icp_defaults(ba_icp_options& o) {
  o.max_iterations = 10; o.max_corr_dist = std::numeric_limits<float>::infinity();
  o.mse_abs_eps = 1e-12; o.mse_rel_eps = 0.0; o.transformation_eps = 0.0;
  o.min_correspondences = 3; o.with_scale = 0; o.fitness_max_range = std::numeric_limits<float>::infinity();
  o.route = BA_ICP_ROUTE_AUTO; o.cell = 0.0f; o.reserved = 0;
}

inline bool icp_finite(float v) { return v - v == 0.0f; }

// Everything the kernels index with or branch on, checked on the host; the
// options are returned with the defaults applied.
inline ba_icp_options check_icp(const char* fn, const ba_icp_batch* b, const ba_icp_options* opt) {
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + what}; };
  if (!b || b->n_sets < 0 || b->n_pairs < 0) throw invalid("bad batch");
  ba_icp_options p;
  if (opt) p = *opt; else icp_defaults(p);
  if (p.max_iterations < 1 || p.max_iterations > 10000) throw invalid("max_iterations must be in 1 .. 10000");
  if (p.min_correspondences < 3) throw invalid("min_correspondences must be at least 3");
  if (!(p.max_corr_dist >= 0.0f)) throw invalid("max_corr_dist must be non-negative");
  if (!(p.fitness_max_range >= 0.0f)) throw invalid("fitness_max_range must be non-negative");
  if (!(p.cell >= 0.0f) || !icp_finite(p.cell)) throw invalid("cell must be non-negative and finite");
  if (p.mse_abs_eps != p.mse_abs_eps || p.mse_rel_eps != p.mse_rel_eps || p.transformation_eps != p.transformation_eps)
    throw invalid("an epsilon is NaN");
  if (p.with_scale != 0 && p.with_scale != 1) throw invalid("unknown with_scale " + std::to_string(p.with_scale));
  if (p.route < BA_ICP_ROUTE_AUTO || p.route > BA_ICP_ROUTE_BRUTE) throw invalid("unknown route " + std::to_string(p.route));
  if (p.reserved != 0) throw invalid("reserved must be 0");
  if (b->n_sets > 0 && !b->set_offset) throw invalid("null array");
  if (b->n_sets > 0) check_offsets(fn, "set_offset", b->set_offset, b->n_sets, "set");
  const int total = b->n_sets > 0 ? b->set_offset[b->n_sets] : 0;
  if (total > 0 && !b->xyz) throw invalid("null array");
  for (int s = 0; s < b->n_sets; ++s)
    for (int i = b->set_offset[s]; i < b->set_offset[s + 1]; ++i)
      for (int a = 0; a < 3; ++a)
        if (!icp_finite(b->xyz[3 * (size_t)i + a]))
          throw invalid("set " + std::to_string(s) + " point " + std::to_string(i - b->set_offset[s]) + " is not finite");
  if (b->n_pairs > 0 && (!b->pair_src || !b->pair_tgt)) throw invalid("null array");
  for (int i = 0; i < b->n_pairs; ++i) {
    const int ss = b->pair_src[i], st = b->pair_tgt[i];
    if (ss < 0 || ss >= b->n_sets || st < 0 || st >= b->n_sets)
      throw invalid("pair " + std::to_string(i) + " names a set out of range");
    if (b->set_offset[ss + 1] - b->set_offset[ss] < 3)
      throw invalid("pair " + std::to_string(i) + ": source set " + std::to_string(ss) + " has fewer than 3 points");
    if (b->set_offset[st + 1] == b->set_offset[st])
      throw invalid("pair " + std::to_string(i) + ": target set " + std::to_string(st) + " is empty");
    if (b->guess)
      for (int e = 0; e < 12; ++e)
        if (!icp_finite(b->guess[16 * (size_t)i + e])) throw invalid("pair " + std::to_string(i) + ": guess is not finite");
  }
  return p;
}

// The grid of one target set: the geometry into G, the counting sort into
// sorted[0 .. nt) and the cell_start run appended to cs.  The cell edge aims
// at kIcpCellPts points per cell of the bounding box (an axis of zero extent
// has one layer and does not count) and shrinks while the occupied cells hold
// more than twice that, or is `cell` when that is positive; it grows until the
// grid holds at most kIcpMaxCells cells.
inline void icp_make_grid(const float* xyz, int nt, float cell, IcpGrid& G, IcpPt* sorted, std::vector<int32_t>& cs) {
  float mn[3], mx[3];
  for (int a = 0; a < 3; ++a) mn[a] = mx[a] = xyz[a];
  for (int i = 1; i < nt; ++i)
    for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], xyz[3 * (size_t)i + a]); mx[a] = std::max(mx[a], xyz[3 * (size_t)i + a]); }
  double e[3], vol = 1.0, emax = 0.0;
  int d = 0;
  for (int a = 0; a < 3; ++a) {
    e[a] = (double)mx[a] - (double)mn[a];
    if (e[a] > 0.0) { vol *= e[a]; ++d; emax = std::max(emax, e[a]); }
    G.mn[a] = mn[a];
    G.c0[a] = (float)(0.5 * ((double)mn[a] + (double)mx[a]));
  }
  double h = cell > 0.0f ? (double)cell : d == 0 ? 1.0 : std::pow(vol * kIcpCellPts / (double)nt, 1.0 / d);
  float hf = (float)h;
  if (!(hf > 0.0f) || !icp_finite(hf)) hf = emax > 0.0 && (float)emax > 0.0f && icp_finite((float)emax) ? (float)emax : 1.0f;
  G.pad = 0;
  G.cell0 = (int32_t)cs.size();
  std::vector<int32_t> cell_of((size_t)nt);
  size_t nc = 0;
  int32_t* start = nullptr;
  for (int pass = 0;; ++pass) {
    for (;;) {
      double cells = 1.0;
      for (int a = 0; a < 3; ++a) cells *= std::floor(e[a] / (double)hf) + 1.0;
      if (cells <= (double)kIcpMaxCells) break;
      hf *= 1.26f;
    }
    G.h = hf;
    for (int a = 0; a < 3; ++a) G.n[a] = (int32_t)(std::floor(e[a] / (double)hf) + 1.0);
    nc = (size_t)G.n[0] * G.n[1] * G.n[2];
    cs.resize((size_t)G.cell0);
    cs.resize((size_t)G.cell0 + nc + 1, 0);
    start = cs.data() + G.cell0;
    size_t occupied = 0;
    for (int i = 0; i < nt; ++i) {
      const float* q = xyz + 3 * (size_t)i;
      const int c = (icp_cell(q[2], mn[2], hf, G.n[2]) * G.n[1] + icp_cell(q[1], mn[1], hf, G.n[1])) * G.n[0] +
                    icp_cell(q[0], mn[0], hf, G.n[0]);
      cell_of[(size_t)i] = c;
      occupied += start[c + 1]++ == 0;
    }
    // A surface fills few cells of its box: while the occupied cells hold more than twice the aim, shrink the
    // edge as for a sheet (occupied cells grow with 1 / h^2) and bin again, three times at the most.
    if (cell > 0.0f || pass == 3 || (double)nt <= 2.0 * kIcpCellPts * (double)occupied) break;
    const float next = hf * (float)std::sqrt((double)kIcpCellPts * (double)occupied / (double)nt);
    if (!(next > 0.0f) || !(next < hf)) break;
    hf = next;
  }
  for (size_t c = 0; c < nc; ++c) start[c + 1] += start[c];
  std::vector<int32_t> fill(start, start + nc);
  for (int i = 0; i < nt; ++i) {
    const float* q = xyz + 3 * (size_t)i;
    sorted[fill[(size_t)cell_of[(size_t)i]]++] = IcpPt{q[0], q[1], q[2], i};
  }
}

// The grids (one per set that a pair of the plan names as its target, built
// once), the pair table, and per GRID pair the permutation that walks the
// source in the cell order of its initial position, so that a wavefront's
// lanes visit the same cells (results are written at the original index).
struct IcpPlan {
  std::vector<IcpPair> pair;
  std::vector<IcpGrid> grid;
  std::vector<int32_t> cell_start;
  std::vector<IcpPt> sorted;         // [points of all sets]; filled for the target sets
  std::vector<int32_t> perm;         // [NS]
  size_t NS = 0, NB = 0;             // source slots, block partials
  int max_ns = 0;
};
inline IcpPlan icp_plan(const char* fn, const ba_icp_batch* b, const ba_icp_options& p, int first_pair, int n_pairs) {
  IcpPlan M;
  const size_t total = b->n_sets > 0 ? (size_t)b->set_offset[b->n_sets] : 0;
  M.sorted.assign(total, IcpPt{0.0f, 0.0f, 0.0f, 0});
  std::vector<int32_t> grid_of((size_t)std::max(b->n_sets, 0), -1);
  M.pair.resize((size_t)n_pairs);
  for (int i = 0; i < n_pairs; ++i) {
    IcpPair& P = M.pair[(size_t)i];
    const int ss = b->pair_src[first_pair + i], st = b->pair_tgt[first_pair + i];
    P.s0 = b->set_offset[ss]; P.ns = b->set_offset[ss + 1] - P.s0;
    P.t0 = b->set_offset[st]; P.nt = b->set_offset[st + 1] - P.t0;
    if (grid_of[(size_t)st] < 0) {
      grid_of[(size_t)st] = (int32_t)M.grid.size();
      M.grid.emplace_back();
      icp_make_grid(b->xyz + 3 * (size_t)P.t0, P.nt, p.cell, M.grid.back(), M.sorted.data() + P.t0, M.cell_start);
    }
    P.grid = grid_of[(size_t)st];
    P.route = p.route != BA_ICP_ROUTE_AUTO ? p.route : P.nt <= kIcpBruteMax ? BA_ICP_ROUTE_BRUTE : BA_ICP_ROUTE_GRID;
    P.soff = (int32_t)M.NS; P.boff = (int32_t)M.NB;
    M.NS += (size_t)P.ns; M.NB += ((size_t)P.ns + kIcpThreads - 1) / kIcpThreads;
    M.max_ns = std::max(M.max_ns, P.ns);
    if (M.NS > 0x7fffffffull || M.cell_start.size() > 0x7fffffffull)
      throw BaError{BA_ERR_INVALID_ARGUMENT, std::string(fn) + "the pairs hold more than 2^31 - 1 source points or cells"};
  }
  M.perm.resize(M.NS);
  std::vector<std::pair<int32_t, int32_t>> order;
  for (int i = 0; i < n_pairs; ++i) {
    const IcpPair& P = M.pair[(size_t)i];
    int32_t* perm = M.perm.data() + P.soff;
    if (P.route != BA_ICP_ROUTE_GRID) {
      for (int q = 0; q < P.ns; ++q) perm[q] = q;
      continue;
    }
    const IcpGrid& G = M.grid[(size_t)P.grid];
    const float ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float* g = b->guess ? b->guess + 16 * (size_t)(first_pair + i) : ident;
    const float Mg[9] = {g[0], g[1], g[2], g[4], g[5], g[6], g[8], g[9], g[10]}, tg[3] = {g[3], g[7], g[11]};
    order.resize((size_t)P.ns);
    for (int q = 0; q < P.ns; ++q) {
      const float* s = b->xyz + 3 * ((size_t)P.s0 + q);
      float x = s[0], y = s[1], z = s[2];
      icp_apply(Mg, tg, x, y, z);
      const int c = (icp_cell(z, G.mn[2], G.h, G.n[2]) * G.n[1] + icp_cell(y, G.mn[1], G.h, G.n[1])) * G.n[0] +
                    icp_cell(x, G.mn[0], G.h, G.n[0]);
      order[(size_t)q] = {c, q};
    }
    std::sort(order.begin(), order.end());
    for (int q = 0; q < P.ns; ++q) perm[q] = order[(size_t)q].second;
  }
  return M;
}

// The staging buffer: pair table, grids, cell_start, cell-sorted targets,
// permutations, states (downloaded on their own), cur (the sources, pair by
// pair), xyz | mse (or ba_icp_nn: idx, d2) | idx, d2, flagged queries, block
// partials.
struct IcpLayout {
  SectionLayout L{256};
  size_t pair = 0, grid = 0, cell_start = 0, sorted = 0, perm = 0, st = 0, cur = 0, xyz = 0;
  size_t mse = 0, idx = 0, d2 = 0, flag = 0, part = 0;
};
inline IcpLayout icp_layout(const IcpPlan& M, size_t total, int max_iter, bool nn) {
  IcpLayout P;
  SectionLayout& L = P.L;
  const size_t N = M.pair.size();
  P.pair = L.add(sizeof(IcpPair) * N); P.grid = L.add(sizeof(IcpGrid) * M.grid.size());
  P.cell_start = L.add(sizeof(int32_t) * M.cell_start.size()); P.sorted = L.add(sizeof(IcpPt) * total);
  P.perm = L.add(sizeof(int32_t) * M.NS); P.st = L.add(sizeof(IcpState) * N); P.cur = L.add(sizeof(float) * 3 * M.NS);
  P.xyz = L.add(sizeof(float) * 3 * total);   // the last input: uploaded from the caller's array
  L.end_inputs();
  if (nn) {
    P.idx = L.add(sizeof(int32_t) * M.NS); P.d2 = L.add(sizeof(float) * M.NS);
    L.end_outputs();
  } else {
    P.mse = L.add(sizeof(double) * N * (size_t)max_iter);
    L.end_outputs();
    P.idx = L.add(sizeof(int32_t) * M.NS); P.d2 = L.add(sizeof(float) * M.NS);
  }
  P.flag = L.add(sizeof(int32_t) * M.NS); P.part = L.add(sizeof(double) * kIcpSums * M.NB);
  return P;
}

// One problem of ba_solve_window_batch as the kernel (ba_window.hip) reads it
struct WinProb {
  int cam0, pt0, obs0;             // first camera / point / observation of the problem in the concatenated arrays
  int nc, np, no, nvc;
  int vc0;                         // first compact variable camera (sum of nvc of the problems before)
  int poff0;                       // pt_off + poff0: [np + 1] CSR of the observations by point
  int coff0;                       // cam_off + coff0: [nvc + 1] CSR of cam_obs by compact variable camera
  int vobs0;                       // cam_obs + vobs0: observations of variable cameras, grouped by camera
  int pad;
};

// The structure of a window batch: the index arrays of WinArgs (ba_kernels.h documents them)
struct WindowPack {
  std::vector<WinProb> prob;
  std::vector<int> cam_vc, pt_off, obs_cam, obs_slot, cam_off, cam_obs;
  std::vector<uint8_t> pt_var;
  std::vector<float> uv;
  size_t NV = 0;                   // compact variable cameras of the whole batch
};

// Per problem: validate, find the variable observed cameras (compact columns
// in increasing camera index) and the variable points, sort the observations
// by (point, camera) as set_problem does (stable), build the point CSR, the
// (point, camera) group heads and the camera CSR.
// (static: as weak symbols of the shared library the sort's instantiations make the build 4 % slower)
static inline WindowPack pack_window_structure(const ba_window_batch& b) {
  const char* const fn = "ba_solve_window_batch: ";   // (a std::string only where an error is raised)
  auto invalid = [&](const std::string& what) { return BaError{BA_ERR_INVALID_ARGUMENT, fn + what}; };
  const int n = b.n_problems;
  if (n < 0) throw invalid("bad batch");
  if (n == 0) return WindowPack{};
  if (!b.cam_offset || !b.pt_offset || !b.obs_offset) throw invalid("null offset array");
  check_offsets(fn, "cam_offset", b.cam_offset, n);
  check_offsets(fn, "pt_offset", b.pt_offset, n);
  check_offsets(fn, "obs_offset", b.obs_offset, n);
  const size_t NC = b.cam_offset[n], NP = b.pt_offset[n], NO = b.obs_offset[n];
  if (NO && (!b.obs_cam || !b.obs_pt || !b.obs_uv)) throw invalid("null array");
  std::vector<WinProb> prob(n);
  std::vector<int> cam_vc(NC, -1), pt_off(NP + n, 0), obs_cam(NO), obs_slot(NO, -1), cam_off, cam_obs;
  std::vector<uint8_t> pt_var(NP, 0);
  std::vector<float> uv(2 * NO);
  std::vector<int> order, cnt;
  size_t NV = 0;
  cam_obs.reserve(NO);
  for (int i = 0; i < n; ++i) {
    WinProb& q = prob[i];
    q = WinProb{};
    q.cam0 = b.cam_offset[i]; q.pt0 = b.pt_offset[i]; q.obs0 = b.obs_offset[i];
    q.nc = b.cam_offset[i + 1] - q.cam0; q.np = b.pt_offset[i + 1] - q.pt0; q.no = b.obs_offset[i + 1] - q.obs0;
    const int32_t* oc = b.obs_cam + q.obs0;
    const int32_t* op = b.obs_pt + q.obs0;
    for (int k = 0; k < q.no; ++k)
      if (oc[k] < 0 || oc[k] >= q.nc || op[k] < 0 || op[k] >= q.np)
        throw invalid("problem " + std::to_string(i) + ": observation " + std::to_string(k) +
                      " has a local index out of range");
    auto cfix = [&](int c) { return b.cam_fixed && b.cam_fixed[q.cam0 + c]; };
    auto pfix = [&](int p) { return b.pt_fixed && b.pt_fixed[q.pt0 + p]; };
    // variable blocks that some residual touches
    int* vc = cam_vc.data() + q.cam0;
    for (int k = 0; k < q.no; ++k) {
      if (!cfix(oc[k])) vc[oc[k]] = 0;
      if (!pfix(op[k])) pt_var[q.pt0 + op[k]] = 1;
    }
    int nvc = 0;
    for (int c = 0; c < q.nc; ++c) if (vc[c] == 0) vc[c] = nvc++;
    if (nvc > BA_WINDOW_MAX_CAMS)
      throw invalid("problem " + std::to_string(i) + " has " + std::to_string(nvc) +
                    " variable observed cameras (at most " + std::to_string(BA_WINDOW_MAX_CAMS) + ")");
    q.nvc = nvc;
    q.vc0 = (int)NV;
    NV += nvc;
    // observations by (point, camera), stable
    order.resize(q.no);
    for (int k = 0; k < q.no; ++k) order[k] = k;
    // (the two pointers by value: by reference the comparator reloads them through the closure, and how
    // well the compiler sees through that depends on what it inlines around this function: 2 ms per 256 windows)
    std::stable_sort(order.begin(), order.end(), [op, oc](int x, int y) {
      return op[x] != op[y] ? op[x] < op[y] : oc[x] < oc[y];
    });
    q.poff0 = q.pt0 + i;
    int* po = pt_off.data() + q.poff0;
    for (int k = 0; k < q.no; ++k) po[op[k] + 1]++;
    for (int p = 0; p < q.np; ++p) po[p + 1] += po[p];
    q.coff0 = (int)cam_off.size();
    q.vobs0 = (int)cam_obs.size();
    cnt.assign(nvc + 1, 0);
    for (int k = 0; k < q.no; ++k) {
      const int src = order[k], c = oc[src], p = op[src];
      obs_cam[q.obs0 + k] = c;
      uv[2 * ((size_t)q.obs0 + k)] = b.obs_uv[2 * ((size_t)q.obs0 + src)];
      uv[2 * ((size_t)q.obs0 + k) + 1] = b.obs_uv[2 * ((size_t)q.obs0 + src) + 1];
      if (vc[c] >= 0) {
        cnt[vc[c] + 1]++;
        const bool head = k == 0 || op[order[k - 1]] != p || oc[order[k - 1]] != c;
        if (head && pt_var[q.pt0 + p]) obs_slot[q.obs0 + k] = vc[c];
      }
    }
    for (int v = 0; v < nvc; ++v) cnt[v + 1] += cnt[v];
    cam_off.insert(cam_off.end(), cnt.begin(), cnt.end());
    cam_obs.resize(q.vobs0 + cnt[nvc]);
    for (int k = 0; k < q.no; ++k) {
      const int v = vc[obs_cam[q.obs0 + k]];
      if (v >= 0) cam_obs[q.vobs0 + cnt[v]++] = k;
    }
  }
  return WindowPack{std::move(prob),    std::move(cam_vc),  std::move(pt_off), std::move(obs_cam), std::move(obs_slot),
                    std::move(cam_off), std::move(cam_obs), std::move(pt_var), std::move(uv),      NV};
}

// ba_iteration records per problem: one per iteration and the initial one;
// refused when the logs of the batch would pass 2^40 bytes
static inline size_t window_log_cap(const char* fn, int max_num_iterations, int n_problems) {
  const size_t log_cap = (size_t)std::max(max_num_iterations, 0) + 1;
  if (log_cap > (size_t(1) << 40) / (sizeof(ba_iteration) * (size_t)n_problems))
    throw BaError{BA_ERR_OUT_OF_MEMORY, std::string(fn) + "the iteration logs do not fit (max_num_iterations x n_problems)"};
  return log_cap;
}

// doubles per camera table row, value-only camera record and observation
// record of the scratch (= kTblRec, kRecL, kJR of the device headers)
constexpr int kWinTbl = 42, kWinVRec = 48, kWinJR = 20;

// The staging buffer: the problems, parameters and structure | parameters,
// summary records, iteration logs | the kernel's scratch (WinArgs documents it)
struct WindowLayout {
  SectionLayout L{256};
  size_t prob = 0, cams = 0, pts = 0, K = 0, extr = 0, vc = 0, pv = 0, poff = 0, oc = 0, slot = 0, uv = 0, coff = 0, cobs = 0;
  size_t cams_out = 0, pts_out = 0, summ = 0, log = 0;
  size_t w_pts = 0, w_ctab = 0, w_vrec = 0, w_JR = 0, w_Hp = 0, w_sp = 0, w_prec = 0, w_W = 0, w_hc = 0;
};
static inline WindowLayout window_layout(const WindowPack& w, size_t log_cap) {
  WindowLayout P;
  SectionLayout& L = P.L;
  const size_t n = w.prob.size(), NC = w.cam_vc.size(), NP = w.pt_var.size(), NO = w.obs_cam.size(), NV = w.NV;
  P.prob = L.add(sizeof(WinProb) * n); P.cams = L.add(sizeof(double) * 6 * NC); P.pts = L.add(sizeof(double) * 3 * NP);
  P.K = L.add(sizeof(float) * 9 * NC); P.extr = L.add(sizeof(float) * 16 * NC); P.vc = L.add(sizeof(int) * NC);
  P.pv = L.add(NP); P.poff = L.add(sizeof(int) * (NP + n)); P.oc = L.add(sizeof(int) * NO); P.slot = L.add(sizeof(int) * NO);
  P.uv = L.add(sizeof(float) * 2 * NO); P.coff = L.add(sizeof(int) * w.cam_off.size());
  P.cobs = L.add(sizeof(int) * w.cam_obs.size());
  L.end_inputs();
  P.cams_out = L.add(sizeof(double) * 6 * NC); P.pts_out = L.add(sizeof(double) * 3 * NP);
  P.summ = L.add(sizeof(double) * 8 * n); P.log = L.add(sizeof(ba_iteration) * log_cap * n);
  L.end_outputs();
  P.w_pts = L.add(sizeof(double) * 6 * NP); P.w_ctab = L.add(sizeof(double) * 2 * kWinTbl * NC);
  P.w_vrec = L.add(sizeof(double) * kWinVRec * NC); P.w_JR = L.add(sizeof(double) * 2 * kWinJR * NO);
  P.w_Hp = L.add(sizeof(double) * 18 * NP); P.w_sp = L.add(sizeof(double) * 3 * NP);
  P.w_prec = L.add(sizeof(double) * 9 * NP); P.w_W = L.add(sizeof(double) * 18 * NO); P.w_hc = L.add(sizeof(double) * 54 * NV);
  return P;
}

}  // namespace bahip
