// ba_batch.hip — the batch entry points of the extern "C" ABI
// (include/ba_hip.h): ba_prune, the pose and window batches, triangulation,
// PnP, two-view, descriptor matching, map-point upkeep and association, the
// map graph and ICP, with their *_defaults, *_times and inspection entries.
// None touches the context's current problem.  Host code only.
//
// Every entry has the same shape: a check_* and a *_layout of
// host/ba_batch_pack.hpp (plain C++, run under sanitizers on the host), then
// the protocol of StagingArena (ba_ctx.h): begin, put the sections, upload,
// the launches of the feature's kernel file, download, copy out.  A new batch
// feature supplies a validator, a layout, an argument struct and such an
// entry.
#include <cfloat>

#include "ba_ctx.h"

using namespace bahip;

extern "C" {

int ba_prune(ba_ctx* ctx, const ba_prune_problem* p, uint8_t* result) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    check_prune(p, result);
    const size_t NC = p->n_cams, NO = p->n_obs;
    if (NO == 0) return;
    const PruneLayout P = prune_layout(NC, NO);
    StagingArena S;   // (call-local: ba_prune keeps no memory between calls)
    S.begin(ctx, P.L, "ba_prune: ");
    S.put(P.extr, p->extr, sizeof(float) * 16 * NC); S.put(P.ctr, p->cam_center, sizeof(float) * 3 * NC);
    S.put(P.K, p->K, sizeof(float) * 9 * NC); S.put(P.X, p->obs_X, sizeof(float) * 3 * NO);
    S.put(P.uv, p->obs_uv, sizeof(float) * 2 * NO); S.put(P.sig, p->obs_inv_sigma, sizeof(float) * NO);
    S.put(P.dist, p->obs_dist, sizeof(float) * 2 * NO); S.put(P.cam, p->obs_cam, sizeof(int) * NO);
    S.upload(P.L.in_b);
    launch_prune(p->n_obs, S.d<const float>(P.extr), S.d<const float>(P.ctr), S.d<const float>(P.K), S.d<const int>(P.cam),
                 S.d<const float>(P.X), S.d<const float>(P.uv), S.d<const float>(P.sig), S.d<const float>(P.dist),
                 S.d<uint8_t>(P.res), ctx->stream);
    HIP_OK(hipGetLastError());
    S.fetch(P.res, NO, result);
    HIP_OK(hipStreamSynchronize(ctx->stream));
  });
}

int ba_solve_pose_batch(ba_ctx* ctx, const ba_pose_batch* b, const ba_options* opt, double* cams_out,
                        ba_summary* summaries) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_solve_pose_batch: ";
    check_pose_batch(fn.c_str(), b, cams_out);
    const int n = b->n_problems;
    if (n == 0) return;
    const size_t N = n, NO = b->obs_offset[n];
    const PoseOpts po = pose_opts(options_or_default(opt));
    StagingArena& S = ctx->pose;
    const double t0 = now_s();
    const PoseLayout P = pose_layout(N, NO);
    S.begin(ctx, P.L, fn);
    S.put(P.off, b->obs_offset, sizeof(int) * (N + 1)); S.put(P.cam, b->cams, sizeof(double) * 6 * N);
    S.put(P.K, b->K, sizeof(float) * 9 * N); S.put(P.X, b->pts, sizeof(double) * 3 * NO);
    S.put(P.uv, b->obs_uv, sizeof(float) * 2 * NO);
    S.upload(P.L.in_b);
    launch_pose_batch(n, S.d<const int>(P.off), S.d<const double>(P.cam), S.d<const float>(P.K), S.d<const double>(P.X),
                      S.d<const float2>(P.uv), b->huber_a, po, S.d<double>(P.out), S.d<double>(P.summ), ctx->stream);
    S.download();
    S.copy_out(cams_out, P.out, sizeof(double) * 6 * N);
    if (summaries) {
      const double wall = now_s() - t0;
      for (size_t i = 0; i < N; ++i) summaries[i] = unpack_summary(S.h<double>(P.summ) + 8 * i, wall, false);
    }
  });
}

// ---------------------------------------------------------------------------
// ba_solve_window_batch.  The structure of every problem
// (pack_window_structure), one upload, one launch (ba_window.hip), one
// download.
// ---------------------------------------------------------------------------
int ba_solve_window_batch(ba_ctx* ctx, const ba_window_batch* b, const ba_options* opt, double* cams_out,
                          double* pts_out, ba_summary* summaries) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_solve_window_batch: ";
    if (!b || b->n_problems < 0) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "bad batch"};
    const ba_options o = options_or_default(opt);
    if (o.linear_solver != BA_DENSE_SCHUR) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "linear_solver must be BA_DENSE_SCHUR"};
    if (o.precision != BA_FP64) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "precision must be BA_FP64"};
    StagingArena& S = ctx->win;
    S.tic();
    const WindowPack w = pack_window_structure(*b);
    const int n = b->n_problems;
    const size_t NC = w.cam_vc.size(), NP = w.pt_var.size(), NO = w.obs_cam.size();
    if ((NC && (!b->cams || !b->K || !cams_out)) || (NP && (!b->pts || !pts_out)))
      throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null array"};
    if (n == 0) {
      ctx->win_log.clear();
      ctx->win_log_n.clear();
      return;
    }
    // the launch's dynamic LDS: the largest over the problems (not monotone in nvc)
    size_t lds = 0;
    for (const WinProb& q : w.prob) lds = std::max(lds, window_lds_bytes(q.nvc));
    const size_t log_cap = window_log_cap(fn.c_str(), o.max_num_iterations, n);
    const WindowLayout P = window_layout(w, log_cap);
    S.begin(ctx, P.L, fn);
    S.put(P.prob, w.prob.data(), sizeof(WinProb) * n); S.put(P.cams, b->cams, sizeof(double) * 6 * NC);
    S.put(P.pts, b->pts, sizeof(double) * 3 * NP); S.put(P.K, b->K, sizeof(float) * 9 * NC);
    S.put(P.extr, b->cam_fixed_extr, sizeof(float) * 16 * NC);   // (null: zeros)
    S.put(P.vc, w.cam_vc.data(), sizeof(int) * NC); S.put(P.pv, w.pt_var.data(), NP);
    S.put(P.poff, w.pt_off.data(), sizeof(int) * (NP + n)); S.put(P.oc, w.obs_cam.data(), sizeof(int) * NO);
    S.put(P.slot, w.obs_slot.data(), sizeof(int) * NO); S.put(P.uv, w.uv.data(), sizeof(float) * 2 * NO);
    S.put(P.coff, w.cam_off.data(), sizeof(int) * w.cam_off.size());
    S.put(P.cobs, w.cam_obs.data(), sizeof(int) * w.cam_obs.size());
    S.upload(P.L.in_b);
    WinArgs A{};
    A.prob = S.d<const WinProb>(P.prob);
    A.NC = NC; A.NP = NP; A.NO = NO; A.NV = w.NV;
    A.log_cap = (int)std::min<size_t>(log_cap, 0x7fffffff);
    A.huber_a = b->huber_a;
    A.cams_in = S.d<double>(P.cams); A.pts_in = S.d<double>(P.pts);
    A.K = S.d<const float>(P.K); A.extr = S.d<const float>(P.extr);
    A.cam_vc = S.d<const int>(P.vc); A.pt_var = S.d<const uint8_t>(P.pv);
    A.pt_off = S.d<const int>(P.poff); A.obs_cam = S.d<const int>(P.oc); A.obs_slot = S.d<const int>(P.slot);
    A.uv = S.d<const float2>(P.uv);
    A.cam_off = S.d<const int>(P.coff); A.cam_obs = S.d<const int>(P.cobs);
    A.pts = S.d<double>(P.w_pts); A.ctab = S.d<double>(P.w_ctab); A.vrec = S.d<double>(P.w_vrec);
    A.JR = S.d<double>(P.w_JR); A.Hp = S.d<double>(P.w_Hp); A.scale_p = S.d<double>(P.w_sp);
    A.prec = S.d<double>(P.w_prec); A.Wb = S.d<double>(P.w_W); A.hc = S.d<double>(P.w_hc);
    A.cams_out = S.d<double>(P.cams_out); A.pts_out = S.d<double>(P.pts_out); A.summ = S.d<double>(P.summ);
    A.log = S.d<char>(P.log);
    const PoseOpts po = pose_opts(o);
    S.kernels_begin();
    HIP_OK((hipError_t)launch_window_batch(n, A, po, lds, ctx->stream));
    S.kernels_end();
    S.download();
    S.copy_out(cams_out, P.cams_out, sizeof(double) * 6 * NC); S.copy_out(pts_out, P.pts_out, sizeof(double) * 3 * NP);
    const double* sm = S.h<double>(P.summ);
    ctx->win_log_cap = A.log_cap;
    ctx->win_log_n.resize(n);
    const ba_iteration* lg = S.h<ba_iteration>(P.log);
    ctx->win_log.assign(lg, lg + log_cap * n);
    const double wall = S.finish();
    for (int i = 0; i < n; ++i) {
      ctx->win_log_n[i] = (int)sm[8 * i + 6];
      if (summaries) summaries[i] = unpack_summary(sm + 8 * i, wall, true);
    }
  });
}

int ba_get_window_iteration_log(ba_ctx* ctx, int problem, ba_iteration* out, int n) {
  if (!ctx || problem < 0 || problem >= (int)ctx->win_log_n.size()) return -BA_ERR_INVALID_ARGUMENT;
  const int avail = ctx->win_log_n[problem];
  const int k = std::min(n, avail);
  if (out && k > 0)
    std::memcpy(out, ctx->win_log.data() + (size_t)problem * ctx->win_log_cap, sizeof(ba_iteration) * k);
  return avail;
}

// the *_times getters: the times the entry's arena kept of its last timed call
int ba_window_times(ba_ctx* ctx, double* ms, int n) { return ctx ? copy_times(ctx->win.ms, ms, n) : -BA_ERR_INVALID_ARGUMENT; }
int ba_triangulate_times(ba_ctx* ctx, double* ms, int n) { return ctx ? copy_times(ctx->tri.ms, ms, n) : -BA_ERR_INVALID_ARGUMENT; }
int ba_pnp_times(ba_ctx* ctx, double* ms, int n) { return ctx ? copy_times(ctx->pnp.ms, ms, n) : -BA_ERR_INVALID_ARGUMENT; }
int ba_two_view_times(ba_ctx* ctx, double* ms, int n) { return ctx ? copy_times(ctx->tv.ms, ms, n) : -BA_ERR_INVALID_ARGUMENT; }
int ba_match_times(ba_ctx* ctx, double* ms, int n) { return ctx ? copy_times(ctx->match.ms, ms, n) : -BA_ERR_INVALID_ARGUMENT; }
int ba_map_points_times(ba_ctx* ctx, double* ms, int n) { return ctx ? copy_times(ctx->mp.ms, ms, n) : -BA_ERR_INVALID_ARGUMENT; }
int ba_map_graph_times(ba_ctx* ctx, double* ms, int n) { return ctx ? copy_times(ctx->mg.ms, ms, n) : -BA_ERR_INVALID_ARGUMENT; }
int ba_icp_times(ba_ctx* ctx, double* ms, int n) { return ctx ? copy_times(ctx->icp.ms, ms, n) : -BA_ERR_INVALID_ARGUMENT; }

// ---------------------------------------------------------------------------
// ba_triangulate: the prologue + one launch (ba_triangulate.hip)
// ---------------------------------------------------------------------------
void ba_triangulate_defaults(ba_tri_options* opt) {
  if (opt) tri_defaults(*opt);
}

int ba_triangulate(ba_ctx* ctx, const ba_tri_batch* b, const ba_tri_options* topt, const ba_options* opt,
                   double* pts_out, uint8_t* status, ba_summary* summaries) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_triangulate: ";
    const ba_options o = options_or_default(opt);
    const ba_tri_options t = check_triangulate(fn.c_str(), b, topt, o, pts_out, status);
    const int np = b->n_pts, nc = b->n_cams;
    if (np == 0) return;
    const size_t no = (size_t)b->obs_offset[np];
    StagingArena& S = ctx->tri;
    S.tic();
    const bool given = t.init == BA_TRI_INIT_GIVEN, has_ctr = b->cam_center != nullptr, has_scale = b->obs_scale != nullptr;
    const TriLayout P = tri_layout((size_t)nc, (size_t)np, no, has_ctr, has_scale, given);
    S.begin(ctx, P.L, fn);
    S.put(P.extr, b->extr, sizeof(float) * 16 * nc); S.put(P.K, b->K, sizeof(float) * 9 * nc);
    S.put(P.off, b->obs_offset, sizeof(int) * ((size_t)np + 1)); S.put(P.oc, b->obs_cam, sizeof(int) * no);
    S.put(P.uv, b->obs_uv, sizeof(float) * 2 * no);
    if (has_ctr) S.put(P.ctr, b->cam_center, sizeof(float) * 3 * nc);   // (the optional sections exist only when given)
    if (has_scale) S.put(P.sc, b->obs_scale, sizeof(float) * no);
    if (given) S.put(P.init, b->pts_init, sizeof(double) * 3 * np);
    S.upload(P.L.in_b);
    TriArgs A{};
    A.n_pts = np; A.n_cams = nc;
    A.init_given = given; A.refine = t.refine; A.min_views = t.min_views; A.checks = t.checks;
    A.behind_any = t.behind_rule;
    A.huber_a = b->huber_a;
    A.extr = S.d<const float>(P.extr); A.center = has_ctr ? S.d<const float>(P.ctr) : nullptr; A.K = S.d<const float>(P.K);
    A.off = S.d<const int>(P.off); A.obs_cam = S.d<const int>(P.oc); A.uv = S.d<const float2>(P.uv);
    A.scale = has_scale ? S.d<const float>(P.sc) : nullptr;
    A.pts_init = given ? S.d<const double>(P.init) : nullptr;
    A.rec = S.d<double>(P.rec);
    A.pts_out = S.d<double>(P.pts); A.summ = S.d<double>(P.summ); A.status = S.d<uint8_t>(P.st);
    const PoseOpts po = pose_opts(o);
    S.kernels_begin();
    launch_triangulate(A, po, ctx->stream);
    S.kernels_end();
    S.download();
    S.copy_out(pts_out, P.pts, sizeof(double) * 3 * np); S.copy_out(status, P.st, (size_t)np);
    const double wall = S.finish();
    if (summaries)
      for (size_t i = 0; i < (size_t)np; ++i) summaries[i] = unpack_summary(S.h<double>(P.summ) + 6 * i, wall, true);
  });
}

// ---------------------------------------------------------------------------
// ba_pnp_ransac / ba_pnp_hypotheses: the launches of ba_pnp.hip
// ---------------------------------------------------------------------------
void ba_pnp_defaults(ba_pnp_options* opt) {
  if (opt) pnp_defaults(*opt);
}

namespace {

// the batch into the arena and onto the device; the kernel arguments that name
// the inputs
PnpArgs pnp_stage(ba_ctx* ctx, const ba_pose_batch* b, const ba_pnp_options& p, const PnpLayout& P, const std::string& fn) {
  const size_t N = b->n_problems, NO = b->obs_offset[N];
  StagingArena& S = ctx->pnp;
  S.begin(ctx, P.L, fn);
  S.put(P.off, b->obs_offset, sizeof(int) * (N + 1)); S.put(P.prior, b->cams, sizeof(double) * 6 * N);
  S.put(P.K, b->K, sizeof(float) * 9 * N); S.put(P.X, b->pts, sizeof(double) * 3 * NO);
  S.put(P.uv, b->obs_uv, sizeof(float) * 2 * NO);
  S.upload(P.L.in_b);
  PnpArgs A{};
  A.n_prob = (int)N; A.H = p.max_hypotheses;
  A.n_min = std::max(4, p.min_points); A.inl_min = std::max(4, p.min_inliers);
  A.use_prior = p.use_prior; A.refine = p.refine;
  A.seed = p.seed; A.thr2 = p.threshold_px * p.threshold_px; A.huber_a = b->huber_a;
  A.off = S.d<const int>(P.off); A.prior = S.d<const double>(P.prior); A.K = S.d<const float>(P.K);
  A.X = S.d<const double>(P.X); A.uv = S.d<const float2>(P.uv);
  return A;
}

}  // namespace

int ba_pnp_ransac(ba_ctx* ctx, const ba_pose_batch* b, const ba_pnp_options* popt, const ba_options* lm,
                  double* cams_out, uint8_t* inlier, ba_pnp_result* results) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_pnp_ransac: ";
    const ba_options o = options_or_default(lm);
    const ba_pnp_options p = check_pnp(fn.c_str(), b, popt, &o);
    const size_t N = b->n_problems;
    if (N == 0) return;
    const size_t NO = b->obs_offset[N];
    if (!cams_out || (NO > 0 && !inlier)) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    StagingArena& S = ctx->pnp;
    S.tic();
    const int G = pnp_group(N, p.max_hypotheses);
    const PnpLayout P = pnp_layout(N, NO, p.max_hypotheses, G, 0);
    PnpArgs A = pnp_stage(ctx, b, p, P, fn);
    A.G = G;
    A.rec = S.d<double>(P.rec); A.cmask = S.d<uint8_t>(P.cmask); A.cnt = S.d<int>(P.cnt); A.coff = S.d<int>(P.coff);
    A.Xc = S.d<double>(P.Xc); A.uvc = S.d<float2>(P.uvc);
    A.cams_out = S.d<double>(P.cams_out); A.cam_ransac = S.d<double>(P.cam_ransac); A.summ = S.d<double>(P.summ);
    A.res = S.d<int>(P.res); A.inlier = S.d<uint8_t>(P.inlier);
    S.kernels_begin();
    launch_pnp(A, pose_opts(o), ctx->stream);
    S.kernels_end();
    S.download();
    S.copy_out(cams_out, P.cams_out, sizeof(double) * 6 * N); S.copy_out(inlier, P.inlier, NO);
    const double wall = S.finish();
    if (results)
      for (size_t i = 0; i < N; ++i) {
        ba_pnp_result& r = results[i];
        const int* ri = S.h<int>(P.res) + 4 * i;
        r = ba_pnp_result{};
        r.status = ri[0]; r.n_inliers = ri[1]; r.n_inliers_ransac = ri[2]; r.best_hypothesis = ri[3];
        S.copy_out(r.cam_ransac, P.cam_ransac + sizeof(double) * 6 * i, sizeof(double) * 6);
        if (p.refine && (ri[0] == BA_PNP_OK || ri[0] == BA_PNP_REFINE_FAILED))
          r.refine = unpack_summary(S.h<double>(P.summ) + 8 * i, wall, true);
      }
  });
}

int ba_pnp_hypotheses(ba_ctx* ctx, const ba_pose_batch* b, const ba_pnp_options* popt, int problem, int h0, int n,
                      int32_t* sample, int32_t* n_sol, double* Rt, int32_t* count) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_pnp_hypotheses: ";
    const ba_pnp_options p = check_pnp(fn.c_str(), b, popt, nullptr);
    check_hypothesis_range(fn.c_str(), "problem", problem, b->n_problems, h0, n, p.max_hypotheses);
    if (n == 0) return;
    if (!sample || !n_sol || !Rt || !count) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    const int nobs = b->obs_offset[problem + 1] - b->obs_offset[problem];
    const bool prior_only = p.use_prior && h0 == 0 && n == 1;
    if (nobs < 3 && !prior_only)
      throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "problem " + std::to_string(problem) + " has fewer than 3 observations"};
    const size_t N = b->n_problems, NO = b->obs_offset[N];
    const PnpLayout P = pnp_layout(N, NO, p.max_hypotheses, 1, (size_t)n);
    PnpArgs A = pnp_stage(ctx, b, p, P, fn);
    A.G = 1;
    StagingArena& S = ctx->pnp;
    const PnpDebug D{problem, h0, n, S.d<int>(P.dbg_sample), S.d<int>(P.dbg_nsol), S.d<double>(P.dbg_Rt), S.d<int>(P.dbg_count)};
    launch_pnp_hypotheses(A, D, ctx->stream);
    S.download();
    S.copy_out(sample, P.dbg_sample, sizeof(int32_t) * 3 * n); S.copy_out(n_sol, P.dbg_nsol, sizeof(int32_t) * n);
    S.copy_out(Rt, P.dbg_Rt, sizeof(double) * 48 * n); S.copy_out(count, P.dbg_count, sizeof(int32_t) * 4 * n);
  });
}

// ---------------------------------------------------------------------------
// ba_two_view_ransac and its inspection entries: the launches of ba_two_view.hip
// ---------------------------------------------------------------------------
void ba_two_view_defaults(ba_two_view_options* opt) {
  if (opt) two_view_defaults(*opt);
}

namespace {

// the batch into the arena and onto the device; the kernel arguments that name
// the inputs
TvArgs two_view_stage(ba_ctx* ctx, const ba_two_view_batch* b, const ba_two_view_options& p, const TwoViewLayout& P,
                      const std::string& fn) {
  const size_t N = b->n_pairs, NM = b->match_offset[N];
  StagingArena& S = ctx->tv;
  S.begin(ctx, P.L, fn);
  S.put(P.off, b->match_offset, sizeof(int) * (N + 1)); S.put(P.K1, b->K1, sizeof(float) * 9 * N);
  S.put(P.K2, b->K2 ? b->K2 : b->K1, sizeof(float) * 9 * N);
  two_view_pack_matches(b, NM, S.h<float>(P.m));
  S.pad(P.m + sizeof(float) * 4 * NM);
  S.upload(P.L.in_b);
  TvArgs A{};
  A.n_pair = (int)N; A.H = p.max_hypotheses;
  A.n_min = std::max(8, p.min_points); A.inl_min = std::max(8, p.min_inliers); A.good_min = std::max(1, p.min_good);
  A.model = p.model; A.G = 1;
  A.seed = p.seed; A.thr2 = p.threshold_px * p.threshold_px; A.h_ratio = p.h_ratio;
  A.off = S.d<const int>(P.off); A.K1 = S.d<const float>(P.K1); A.K2 = S.d<const float>(P.K2);
  A.m = S.d<const float4>(P.m);
  A.models = S.d<double>(P.models); A.valid = S.d<int>(P.valid);
  return A;
}

// what the two inspection entries check alike, after check_two_view
static void check_two_view_inspection(const std::string& fn, const ba_two_view_batch* b, const ba_two_view_options& p, int pair,
                               int h0, int n, bool outputs) {
  check_hypothesis_range(fn.c_str(), "pair", pair, b->n_pairs, h0, n, p.max_hypotheses);
  if (n == 0) return;
  if (!outputs) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
  if (b->match_offset[pair + 1] - b->match_offset[pair] < 8)
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "pair " + std::to_string(pair) + " has fewer than 8 matches"};
}

}  // namespace

int ba_two_view_ransac(ba_ctx* ctx, const ba_two_view_batch* b, const ba_two_view_options* opt, uint8_t* inlier,
                       ba_two_view_result* results) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_two_view_ransac: ";
    const ba_two_view_options p = check_two_view(fn.c_str(), b, opt);
    const size_t N = b->n_pairs;
    if (N == 0) return;
    const size_t NM = b->match_offset[N];
    if (!results || (NM > 0 && !inlier)) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    StagingArena& S = ctx->tv;
    S.tic();
    const int G = pnp_group(N, p.max_hypotheses);
    const bool e5 = p.reserved == BA_TV_E_FIVE_POINT;
    const int G5 = pnp_group(N, 10 * p.max_hypotheses);   // the vote of the five-point solutions runs over 10 H slots
    const TwoViewLayout P = two_view_layout(N, NM, p.max_hypotheses, G, 0, e5, G5);
    TvArgs A = two_view_stage(ctx, b, p, P, fn);
    A.G = G;
    A.rec = S.d<unsigned long long>(P.rec); A.res = S.d<double>(P.res); A.inlier = S.d<uint8_t>(P.inlier);
    if (e5) {
      A.e5 = 1; A.G5 = G5;
      A.models5 = S.d<double>(P.models5); A.nsol5 = S.d<int>(P.nsol5); A.rec5 = S.d<unsigned long long>(P.rec5);
    }
    S.kernels_begin();
    launch_two_view(A, ctx->stream);
    S.kernels_end();
    S.download();
    S.copy_out(inlier, P.inlier, NM);
    for (size_t i = 0; i < N; ++i) {
      const double* r = S.h<double>(P.res) + (size_t)kTvRes * i;
      ba_two_view_result& o = results[i];
      o = ba_two_view_result{};
      o.status = (int)r[0]; o.model = (int)r[1]; o.n_inliers = (int)r[2]; o.n_good = (int)r[3]; o.n_good_second = (int)r[4];
      o.best_hypothesis_e = (int)r[5]; o.best_hypothesis_h = (int)r[6]; o.votes_e = (int)r[7]; o.votes_h = (int)r[8];
      o.reserved = (int)r[38];
      o.score_e = r[9]; o.score_h = r[10];
      std::memcpy(o.E, r + 11, sizeof(double) * 9);
      std::memcpy(o.H, r + 20, sizeof(double) * 9);
      std::memcpy(o.cam, r + 29, sizeof(double) * 6);
      std::memcpy(o.normal, r + 35, sizeof(double) * 3);
    }
    S.finish();
  });
}

int ba_two_view_hypotheses(ba_ctx* ctx, const ba_two_view_batch* b, const ba_two_view_options* opt, int pair, int h0, int n,
                           int32_t* sample, double* E, double* H, int32_t* valid, int32_t* count) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_two_view_hypotheses: ";
    const ba_two_view_options p = check_two_view(fn.c_str(), b, opt);
    check_two_view_inspection(fn, b, p, pair, h0, n, sample && E && H && valid && count);
    if (n == 0) return;
    const size_t N = b->n_pairs, NM = b->match_offset[N];
    const TwoViewLayout P = two_view_layout(N, NM, p.max_hypotheses, 1, (size_t)n);
    TvArgs A = two_view_stage(ctx, b, p, P, fn);
    A.n_min = 8;
    StagingArena& S = ctx->tv;
    const TvDebug D{pair, h0, n, S.d<int>(P.dbg_sample), S.d<int>(P.dbg_count)};
    launch_two_view_hypotheses(A, D, ctx->stream);
    S.download();
    S.copy_out(sample, P.dbg_sample, sizeof(int32_t) * 8 * n); S.copy_out(valid, P.valid, sizeof(int32_t) * 2 * n);
    S.copy_out(count, P.dbg_count, sizeof(int32_t) * 2 * n);
    const double* m = S.h<double>(P.models);
    for (int i = 0; i < n; ++i) {
      std::memcpy(E + 9 * (size_t)i, m + 18 * (size_t)i, sizeof(double) * 9);
      std::memcpy(H + 9 * (size_t)i, m + 18 * (size_t)i + 9, sizeof(double) * 9);
    }
  });
}

int ba_two_view_hypotheses_e5(ba_ctx* ctx, const ba_two_view_batch* b, const ba_two_view_options* opt, int pair, int h0, int n,
                              int32_t* sample, int32_t* n_sol, double* E, int32_t* count) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_two_view_hypotheses_e5: ";
    const ba_two_view_options p = check_two_view(fn.c_str(), b, opt);
    check_two_view_inspection(fn, b, p, pair, h0, n, sample && n_sol && E && count);
    if (n == 0) return;
    const size_t N = b->n_pairs, NM = b->match_offset[N];
    const TwoViewLayout P = two_view_layout(N, NM, p.max_hypotheses, 1, (size_t)n, true);
    TvArgs A = two_view_stage(ctx, b, p, P, fn);
    A.n_min = 8;
    StagingArena& S = ctx->tv;
    A.e5 = 1; A.G5 = 1;
    A.models = nullptr; A.valid = nullptr;   // (the layout has no eight-point sections)
    A.models5 = S.d<double>(P.models5); A.nsol5 = S.d<int>(P.nsol5);
    TvDebug D{pair, h0, n, S.d<int>(P.dbg_sample), nullptr, S.d<int>(P.dbg_count5)};
    launch_two_view_hypotheses_e5(A, D, ctx->stream);
    S.download();
    S.copy_out(sample, P.dbg_sample, sizeof(int32_t) * 8 * n); S.copy_out(n_sol, P.nsol5, sizeof(int32_t) * n);
    S.copy_out(count, P.dbg_count5, sizeof(int32_t) * 10 * n);
    const double* m = S.h<double>(P.models5);   // [10][n][9] -> [n][10][9]
    for (int i = 0; i < n; ++i)
      for (int sidx = 0; sidx < 10; ++sidx)
        std::memcpy(E + 9 * (10 * (size_t)i + sidx), m + 9 * ((size_t)sidx * n + i), sizeof(double) * 9);
  });
}

// ---------------------------------------------------------------------------
// ba_match_descriptors / ba_match_knn.  The tables go up through the staging
// copy and the descriptors from the caller's array, then the launches of
// ba_match.hip and one download.
// ---------------------------------------------------------------------------
void ba_match_defaults(ba_match_options* opt) {
  if (opt) match_defaults(*opt);
}

namespace {

// the batch (the pairs of the plan) into the arena and onto the device; the
// kernel arguments
MatchArgs match_stage(ba_ctx* ctx, const ba_match_batch* b, const ba_match_options& p, const MatchPlan& M,
                      const MatchLayout& P, bool knn, const std::string& fn) {
  const size_t rows = b->n_sets > 0 ? (size_t)b->set_offset[b->n_sets] : 0, dim = (size_t)b->dim;
  const bool have_ref = b->row_ref != nullptr;
  const size_t n_ref = have_ref ? (size_t)b->n_ref : 0;
  StagingArena& S = ctx->match;
  // The descriptors are the bulk of the batch (125 MB for 256 pairs of 1000 x 1000) and the last input
  // section: they go up from the caller's array, which the call outlives, not through the host copy.
  S.begin(ctx, P.L, fn);
  S.put(P.pair, M.pair.data(), sizeof(MatchPair) * M.pair.size());
  if (have_ref) {
    S.put(P.row_ref, b->row_ref, sizeof(int32_t) * rows); S.put(P.ref, b->ref_desc, sizeof(float) * n_ref * dim);
  }
  S.upload(P.desc);
  S.upload_from(P.desc, b->desc, sizeof(float) * rows * dim);
  MatchArgs A{};
  A.n_pair = (int)M.pair.size(); A.dim = b->dim; A.rows = (int)rows; A.n_ref = (int)n_ref;
  A.max_nq = M.max_nq; A.max_nt = M.max_nt; A.chunks = M.chunks; A.chunk_rows = M.chunk_rows;
  A.select = knn ? 0 : 1; A.unique = p.unique; A.ratio = p.ratio; A.max_distance = p.max_distance;
  A.pair = S.d<const MatchPair>(P.pair); A.desc = S.d<const float>(P.desc);
  A.row_ref = have_ref ? S.d<const int>(P.row_ref) : nullptr; A.ref = S.d<const float>(P.ref);
  A.norms = S.d<float>(P.norms); A.part = S.d<unsigned long long>(P.part); A.knn = S.d<ba_match_neighbors>(P.knn);
  if (!knn) {
    A.surv = S.d<uint8_t>(P.surv); A.win = S.d<unsigned long long>(P.win); A.hist = S.d<int>(P.hist);
    A.cnt = S.d<int>(P.cnt); A.matches = S.d<ba_match>(P.matches);
    if (M.NT) {   // no winner, no survivor yet
      HIP_OK(hipMemsetAsync(A.win, 0xff, sizeof(uint64_t) * M.NT, ctx->stream));
      HIP_OK(hipMemsetAsync(A.hist, 0, sizeof(int32_t) * M.NT, ctx->stream));
    }
  }
  return A;
}

}  // namespace

int ba_match_descriptors(ba_ctx* ctx, const ba_match_batch* b, const ba_match_options* opt, int32_t* match_offset,
                         ba_match* matches) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_match_descriptors: ";
    const ba_match_options p = check_match(fn.c_str(), b, opt);
    if (!match_offset) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    const size_t N = b->n_pairs;
    match_offset[0] = 0;
    if (N == 0) return;
    StagingArena& S = ctx->match;
    S.tic();
    const MatchPlan M = match_plan(fn.c_str(), b, p.unique, 0, (int)N);
    if (M.NM > 0 && !matches) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    const size_t rows = (size_t)b->set_offset[b->n_sets];
    const MatchLayout P = match_layout(M, rows, (size_t)b->n_ref, b->dim, b->row_ref != nullptr, false);
    const MatchArgs A = match_stage(ctx, b, p, M, P, false, fn);
    S.kernels_begin();
    launch_match(A, ctx->stream, S.phase_stamps());   // stamps: after the norms, the 2-NN contraction, the rest
    S.download();
    const int* cnt = S.h<int>(P.cnt);
    const ba_match* rec = S.h<ba_match>(P.matches);
    size_t o = 0;
    for (size_t i = 0; i < N; ++i) {
      const MatchPair& Q = M.pair[i];
      const int c = std::min(std::max(cnt[i], 0), Q.cap);
      if (c) std::memcpy(matches + o, rec + Q.moff, sizeof(ba_match) * (size_t)c);
      o += (size_t)c;
      match_offset[i + 1] = (int32_t)o;
    }
    S.finish_phases(3);
  });
}

int ba_match_knn(ba_ctx* ctx, const ba_match_batch* b, int pair, ba_match_neighbors* out) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_match_knn: ";
    const ba_match_options p = check_match(fn.c_str(), b, nullptr);
    if (pair < 0 || pair >= b->n_pairs)
      throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "pair " + std::to_string(pair) + " out of range"};
    const MatchPlan M = match_plan(fn.c_str(), b, 1, pair, 1);
    if (M.NQ == 0) return;
    if (!out) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    const size_t rows = (size_t)b->set_offset[b->n_sets];
    const MatchLayout P = match_layout(M, rows, (size_t)b->n_ref, b->dim, b->row_ref != nullptr, true);
    const MatchArgs A = match_stage(ctx, b, p, M, P, true, fn);
    launch_match(A, ctx->stream, nullptr);
    ctx->match.download();
    ctx->match.copy_out(out, P.knn, sizeof(ba_match_neighbors) * M.NQ);
  });
}

// ---------------------------------------------------------------------------
// ba_map_points_update / ba_map_points_distances / ba_associate.  The tables go
// up through the staging copy and the descriptors from the caller's arrays,
// then the launches of ba_map_points.hip and one download.
// ---------------------------------------------------------------------------
void ba_map_points_defaults(ba_map_point_options* opt) {
  if (opt) map_points_defaults(*opt);
}
void ba_associate_defaults(ba_assoc_options* opt) {
  if (opt) assoc_defaults(*opt);
}

namespace {

MapPointsArgs map_points_stage(ba_ctx* ctx, const ba_map_point_batch* b, const ba_map_point_options& p,
                               const MapPointsPlan& M, const MapPointsLayout& P, const std::string& fn) {
  const size_t np = (size_t)b->n_pts, no = (size_t)b->obs_offset[np], dim = (size_t)b->dim;
  StagingArena& S = ctx->mp;
  S.begin(ctx, P.L, fn);
  S.put(P.center, b->cam_center, sizeof(float) * 3 * (size_t)b->n_cams); S.put(P.pts, b->pts, sizeof(float) * 3 * np);
  S.put(P.off, b->obs_offset, sizeof(int32_t) * (np + 1)); S.put(P.cam, b->obs_cam, sizeof(int32_t) * no);
  S.put(P.row, b->obs_row, sizeof(int32_t) * no); S.put(P.order, M.order.data(), sizeof(int32_t) * M.order.size());
  if (b->obs_scale) S.put(P.scale, b->obs_scale, sizeof(float) * no);   // (the optional sections exist only when given)
  if (b->ref_obs) S.put(P.ref, b->ref_obs, sizeof(int32_t) * np);
  S.upload(P.desc);
  // the descriptors are the bulk of the batch: they go up from the caller's array, which the call outlives
  if (no > 0) S.upload_from(P.desc, b->desc, sizeof(float) * (size_t)b->n_rows * dim);
  MapPointsArgs A{};
  A.dim = b->dim; A.median_rule = p.median_rule; A.max_scale = p.max_scale;
  for (int t = 0; t < 3; ++t) { A.first[t] = M.first[t]; A.count[t] = M.count[t]; }
  A.center = S.d<const float>(P.center); A.pts = S.d<const float>(P.pts); A.obs_offset = S.d<const int>(P.off);
  A.obs_cam = S.d<const int>(P.cam); A.obs_row = S.d<const int>(P.row);
  A.obs_scale = b->obs_scale ? S.d<const float>(P.scale) : nullptr;
  A.ref_obs = b->ref_obs ? S.d<const int>(P.ref) : nullptr;
  A.desc = S.d<const float>(P.desc); A.order = S.d<const int>(P.order);
  A.out = S.d<ba_map_point>(P.out); A.out_stride = 1;
  return A;
}

}  // namespace

int ba_map_points_update(ba_ctx* ctx, const ba_map_point_batch* b, const ba_map_point_options* opt, ba_map_point* out,
                         float* desc_out) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_map_points_update: ";
    const ba_map_point_options p = check_map_points(fn.c_str(), b, opt);
    const size_t np = (size_t)b->n_pts, dim = (size_t)b->dim;
    if (np == 0) return;
    if (!out) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    StagingArena& S = ctx->mp;
    S.tic();
    const MapPointsPlan M = map_points_plan(b, 0, b->n_pts);
    const MapPointsLayout P = map_points_layout(b, np, desc_out != nullptr, 0);
    MapPointsArgs A = map_points_stage(ctx, b, p, M, P, fn);
    A.desc_out = desc_out ? S.d<float>(P.desc_out) : nullptr;
    S.kernels_begin();
    launch_map_points(A, ctx->stream);
    S.kernels_end();
    S.download();
    S.copy_out(out, P.out, sizeof(ba_map_point) * np); S.copy_out(desc_out, P.desc_out, sizeof(float) * np * dim);
    S.finish();
  });
}

int ba_map_points_distances(ba_ctx* ctx, const ba_map_point_batch* b, int point, float* D, float* m) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_map_points_distances: ";
    ba_map_point_options p = check_map_points(fn.c_str(), b, nullptr);
    if (point < 0 || point >= b->n_pts)
      throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "point " + std::to_string(point) + " out of range"};
    const size_t n = (size_t)(b->obs_offset[point + 1] - b->obs_offset[point]);
    if (n == 0) return;
    if (!D || !m) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    const MapPointsPlan M = map_points_plan(b, point, 1);
    const MapPointsLayout P = map_points_layout(b, 1, false, n);
    MapPointsArgs A = map_points_stage(ctx, b, p, M, P, fn);
    StagingArena& S = ctx->mp;
    A.out_stride = 0;
    A.dbg_D = S.d<float>(P.dbg_D); A.dbg_m = S.d<float>(P.dbg_m);
    launch_map_points(A, ctx->stream);
    S.download();
    S.copy_out(D, P.dbg_D, sizeof(float) * n * n); S.copy_out(m, P.dbg_m, sizeof(float) * n);
  });
}

int ba_associate(ba_ctx* ctx, const ba_assoc_batch* b, const ba_assoc_options* opt, ba_assoc_result* items,
                 ba_fuse_result* fuse) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_associate: ";
    const ba_assoc_options p = check_assoc(fn.c_str(), b, opt);
    const size_t nc = (size_t)b->n_cams, np = (size_t)b->n_pts, ni = (size_t)b->n_items, nf = (size_t)b->n_fuse,
                 dim = (size_t)b->dim;
    if (ni + nf == 0) return;
    if ((ni > 0 && !items) || (nf > 0 && !fuse)) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    if (ni + nf > 0x7fffffffull) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "more than 2^31 - 1 items and fuse pairs"};
    const AssocLayout P = assoc_layout(b);
    StagingArena& S = ctx->mp;
    S.begin(ctx, P.L, fn);
    S.put(P.extr, b->extr, sizeof(float) * 16 * nc); S.put(P.center, b->cam_center, sizeof(float) * 3 * nc);
    S.put(P.K, b->K, sizeof(float) * 9 * nc); S.put(P.size, b->image_size, sizeof(int32_t) * 2 * nc);
    S.put(P.pts, b->pts, sizeof(float) * 3 * np); S.put(P.dir, b->pt_view_dir, sizeof(float) * 3 * np);
    S.put(P.dist, b->pt_dist, sizeof(float) * 2 * np); S.put(P.cam, b->item_cam, sizeof(int32_t) * ni);
    S.put(P.pt, b->item_pt, sizeof(int32_t) * ni); S.put(P.uv, b->item_uv, sizeof(float) * 2 * ni);
    S.put(P.row, b->item_row, sizeof(int32_t) * ni); S.put(P.fuse, b->fuse_pairs, sizeof(int32_t) * 2 * nf);
    if (b->item_scale) S.put(P.scale, b->item_scale, sizeof(float) * ni);   // (the optional sections exist only when given)
    if (b->item_cur_row) S.put(P.cur, b->item_cur_row, sizeof(int32_t) * ni);
    S.upload(P.pt_desc);
    // the two descriptor tables go up from the caller's arrays, which the call outlives
    S.upload_from(P.pt_desc, b->pt_desc, sizeof(float) * np * dim);
    S.upload_from(P.desc, b->desc, sizeof(float) * (size_t)b->n_rows * dim);
    AssocArgs A{};
    A.dim = b->dim; A.n_items = b->n_items; A.n_fuse = b->n_fuse; A.opt = p;
    A.extr = S.d<const float>(P.extr); A.center = S.d<const float>(P.center); A.K = S.d<const float>(P.K);
    A.image_size = S.d<const int>(P.size); A.pts = S.d<const float>(P.pts); A.pt_view_dir = S.d<const float>(P.dir);
    A.pt_dist = S.d<const float>(P.dist); A.pt_desc = S.d<const float>(P.pt_desc); A.desc = S.d<const float>(P.desc);
    A.item_cam = S.d<const int>(P.cam); A.item_pt = S.d<const int>(P.pt); A.item_uv = S.d<const float>(P.uv);
    A.item_scale = b->item_scale ? S.d<const float>(P.scale) : nullptr; A.item_row = S.d<const int>(P.row);
    A.item_cur_row = b->item_cur_row ? S.d<const int>(P.cur) : nullptr; A.fuse_pairs = S.d<const int>(P.fuse);
    A.items = S.d<ba_assoc_result>(P.items); A.fuse = S.d<ba_fuse_result>(P.fused);
    launch_associate(A, ctx->stream);
    S.download();
    S.copy_out(items, P.items, sizeof(ba_assoc_result) * ni); S.copy_out(fuse, P.fused, sizeof(ba_fuse_result) * nf);
  });
}

// ---------------------------------------------------------------------------
// ba_map_graph / ba_map_graph_lists / ba_map_graph_weights.  The table goes up
// from the caller's arrays once; the queries are served in chunks under a
// fixed scratch budget: count launches, the chunk's records to the host, a
// scan there, then the fill launches into the context's list buffers.
// ---------------------------------------------------------------------------
void ba_map_graph_defaults(ba_graph_options* opt) {
  if (opt) map_graph_defaults(*opt);
}

namespace {

// Uploads the table, its frame-sorted view and the queries into ctx->mg and
// returns the kernel arguments with the scratch of the layout's chunk.
MapGraphArgs map_graph_stage(ba_ctx* ctx, const ba_map_table* t, const MapGraphPlan& M, const int32_t* query, int n_query,
                             const ba_graph_options& p, bool want_status, const MapGraphLayout& P, const std::string& fn) {
  const size_t nf = (size_t)t->n_frames, np = (size_t)t->n_pts, no = (size_t)t->n_obs, nq = (size_t)n_query;
  StagingArena& S = ctx->mg;
  S.begin(ctx, P.L, fn);
  S.upload_from(P.frame_id, t->frame_id, 4 * nf); S.upload_from(P.is_key, t->frame_is_key, nf);
  S.upload_from(P.pt_invalid, t->pt_invalid, np);
  if (want_status) S.upload_from(P.pt_ref, t->pt_ref_frame, 4 * np);
  S.upload_from(P.off, t->obs_offset, 4 * (np + 1)); S.upload_from(P.frame, t->obs_frame, 4 * no);
  S.upload_from(P.octave, t->obs_octave, 4 * no); S.upload_from(P.outlier, t->obs_outlier, no);
  S.upload_from(P.obs_pt, M.obs_pt.data(), 4 * no); S.upload_from(P.perm, M.perm.data(), 4 * no);
  S.upload_from(P.frame_off, M.frame_off.data(), 4 * (nf + 1)); S.upload_from(P.query, query, 4 * nq);
  MapGraphArgs A{};
  A.n_frames = t->n_frames; A.n_pts = t->n_pts; A.n_obs = t->n_obs;
  A.th = p.th; A.n_best = p.n_best; A.order = p.order; A.build_windows = p.build_windows ? 1 : 0;
  A.tile = map_graph_tile(p, t->n_frames); A.fraction = p.redundant_fraction;
  A.frame_id = S.d<const int>(P.frame_id);
  A.is_key = t->frame_is_key ? S.d<const uint8_t>(P.is_key) : nullptr;
  A.pt_invalid = t->pt_invalid ? S.d<const uint8_t>(P.pt_invalid) : nullptr;
  A.obs_offset = S.d<const int>(P.off); A.obs_frame = S.d<const int>(P.frame);
  A.obs_octave = t->obs_octave ? S.d<const int>(P.octave) : nullptr;
  A.obs_outlier = t->obs_outlier ? S.d<const uint8_t>(P.outlier) : nullptr;
  A.obs_pt = S.d<const int>(P.obs_pt); A.perm = S.d<const int>(P.perm); A.frame_off = S.d<const int>(P.frame_off);
  A.W = S.d<int>(P.W); A.lst_f = S.d<int>(P.lst_f); A.lst_w = S.d<int>(P.lst_w); A.best = S.d<int>(P.best);
  A.locbits = S.d<unsigned>(P.loc); A.fixbits = S.d<unsigned>(P.fix); A.fixpre = S.d<int>(P.pre);
  A.ptbits = S.d<unsigned>(P.ptb); A.off = S.d<const long long>(P.offs);
  return A;
}

// Room for `need` elements in list array a, keeping the first `keep`
void graph_lists_reserve(ba_ctx* ctx, int a, size_t need, size_t keep, const std::string& fn) {
  GraphLists& G = ctx->graph;
  if (need <= G.cap[a]) return;
  const size_t cap = std::max(need, 2 * G.cap[a]), es = GraphLists::elem[a];
  char* nb = nullptr;
  const hipError_t e = hipMalloc(&nb, cap * es);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    throw BaError{e == hipErrorOutOfMemory ? BA_ERR_OUT_OF_MEMORY : BA_ERR_DEVICE,
                  fn + "lists of " + std::to_string(cap * es) + " bytes: " + hipGetErrorString(e)};
  }
  if (G.buf[a]) {
    if (keep) HIP_OK(hipMemcpyAsync(nb, G.buf[a], keep * es, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    (void)hipFree(G.buf[a]);
  }
  G.buf[a] = nb; G.cap[a] = cap;
}

}  // namespace

int ba_map_graph(ba_ctx* ctx, const ba_map_table* t, const int32_t* query, int n_query, const ba_graph_options* opt,
                 ba_graph_frame* out, uint8_t* pt_status) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_map_graph: ";
    const bool want_status = pt_status != nullptr;
    const ba_graph_options p = check_map_table(fn.c_str(), t, query, n_query, opt, want_status);
    if (n_query > 0 && !out) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    StagingArena& S = ctx->mg;
    S.tic();
    GraphLists& G = ctx->graph;
    G.valid = false;
    for (size_t& l : G.len) l = 0;
    const MapGraphPlan M = map_graph_plan(t);
    const int chunk = map_graph_chunk(p, t, n_query);
    const MapGraphLayout P = map_graph_layout(t, p, n_query, chunk, want_status);
    MapGraphArgs A = map_graph_stage(ctx, t, M, query, n_query, p, want_status, P, fn);
    S.prepared();
    // a group of launches between the arena's stamps; its time is added after the next synchronisation
    auto timed = [&](auto&& launches) {
      S.kernels_begin();
      launches();
      S.kernels_end();
    };
    std::vector<long long> offs;
    for (int c0 = 0; c0 < n_query; c0 += chunk) {
      const int n = std::min(chunk, n_query - c0);
      A.query = S.d<const int>(P.query) + c0; A.rec = S.d<ba_graph_frame>(P.rec) + c0; A.n_chunk = n;
      if (p.build_windows && P.offs > P.loc) HIP_OK(hipMemsetAsync(S.dev + P.loc, 0, P.offs - P.loc, ctx->stream));
      timed([&] { launch_map_graph_count(A, ctx->stream); });
      S.fetch(P.rec + sizeof(ba_graph_frame) * (size_t)c0, sizeof(ba_graph_frame) * (size_t)n, out + c0);
      HIP_OK(hipStreamSynchronize(ctx->stream));
      S.kernels_done();
      offs.resize(4 * (size_t)n);
      size_t len[4] = {G.len[0], G.len[1], G.len[2], G.len[3]};
      for (int i = 0; i < n; ++i) {
        const ba_graph_frame& r = out[c0 + i];
        for (int k = 0; k < 4; ++k) offs[4 * (size_t)i + k] = (long long)len[k];
        len[0] += (size_t)r.degree; len[1] += (size_t)(r.n_local + r.n_fixed); len[2] += (size_t)r.n_win_pts;
        len[3] += (size_t)r.n_win_obs;
      }
      for (int a = 0; a < GraphLists::kArrays; ++a)
        graph_lists_reserve(ctx, a, len[GraphLists::kind[a]], G.len[GraphLists::kind[a]], fn);
      for (int k = 0; k < 4; ++k) G.len[k] = len[k];
      S.upload_from(P.offs, offs.data(), sizeof(long long) * offs.size());
      A.nbr_frame = at<int>(G.buf[0], 0); A.nbr_weight = at<int>(G.buf[1], 0); A.win_cam = at<int>(G.buf[2], 0);
      A.win_cam_fixed = at<uint8_t>(G.buf[3], 0); A.win_pt = at<int>(G.buf[4], 0); A.win_obs = at<int>(G.buf[5], 0);
      A.win_obs_cam = at<int>(G.buf[6], 0); A.win_obs_pt = at<int>(G.buf[7], 0);
      timed([&] { launch_map_graph_fill(A, ctx->stream); });
      HIP_OK(hipStreamSynchronize(ctx->stream));
      S.kernels_done();
    }
    if (want_status && t->n_pts > 0) {
      timed([&] {
        launch_map_graph_status(A, S.d<const int>(P.pt_ref), p.current_frame_id, S.d<uint8_t>(P.status), ctx->stream);
      });
      S.fetch(P.status, (size_t)t->n_pts, pt_status);
      HIP_OK(hipStreamSynchronize(ctx->stream));
      S.kernels_done();
    }
    HIP_OK(hipStreamSynchronize(ctx->stream));
    G.valid = true;
    S.finish();
  });
}

int ba_map_graph_lists(ba_ctx* ctx, const ba_graph_lists* out) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_map_graph_lists: ";
    if (!out) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output"};
    const GraphLists& G = ctx->graph;
    if (!G.valid) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "no ba_map_graph result on this context"};
    void* dst[GraphLists::kArrays] = {out->nbr_frame, out->nbr_weight, out->win_cam, out->win_cam_fixed,
                                      out->win_pt, out->win_obs, out->win_obs_cam, out->win_obs_pt};
    HIP_OK(hipSetDevice(ctx->device));
    for (int a = 0; a < GraphLists::kArrays; ++a) {
      const size_t nb = G.len[GraphLists::kind[a]] * GraphLists::elem[a];
      if (dst[a] && nb) HIP_OK(hipMemcpyAsync(dst[a], G.buf[a], nb, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_OK(hipStreamSynchronize(ctx->stream));
  });
}

int ba_map_graph_weights(ba_ctx* ctx, const ba_map_table* t, int frame, const ba_graph_options* opt, int32_t* W) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_map_graph_weights: ";
    const int32_t q = frame;
    ba_graph_options p = check_map_table(fn.c_str(), t, &q, 1, opt, false);
    if (!W) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    p.build_windows = 0;
    const MapGraphPlan M = map_graph_plan(t);
    const MapGraphLayout P = map_graph_layout(t, p, 1, 1, false);
    MapGraphArgs A = map_graph_stage(ctx, t, M, &q, 1, p, false, P, fn);
    StagingArena& S = ctx->mg;
    A.query = S.d<const int>(P.query); A.n_chunk = 1;
    launch_map_graph_weights(A, ctx->stream);
    HIP_OK(hipGetLastError());
    S.fetch(P.W, sizeof(int32_t) * (size_t)t->n_frames, W);
    HIP_OK(hipStreamSynchronize(ctx->stream));
  });
}

// ---------------------------------------------------------------------------
// ba_icp / ba_icp_nn.  The tables go up through the staging copy and the clouds
// from the caller's array, then max_iterations + 1 rounds of ba_icp.hip with
// no sync in between and one download.
// ---------------------------------------------------------------------------
void ba_icp_defaults(ba_icp_options* opt) {
  if (opt) icp_defaults(*opt);
}

namespace {

// the batch (pairs [first, first + n) of it) into the arena and onto the
// device; the kernel arguments
IcpArgs icp_stage(ba_ctx* ctx, const ba_icp_batch* b, const ba_icp_options& p, const IcpPlan& M, const IcpLayout& P,
                  int first, const std::string& fn) {
  const size_t N = M.pair.size(), total = (size_t)b->set_offset[b->n_sets];
  if (N > 65535) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "more than 65535 pairs"};
  StagingArena& S = ctx->icp;
  S.begin(ctx, P.L, fn);
  S.put(P.pair, M.pair.data(), sizeof(IcpPair) * N); S.put(P.grid, M.grid.data(), sizeof(IcpGrid) * M.grid.size());
  S.put(P.cell_start, M.cell_start.data(), sizeof(int32_t) * M.cell_start.size());
  S.put(P.sorted, M.sorted.data(), sizeof(IcpPt) * total); S.put(P.perm, M.perm.data(), sizeof(int32_t) * M.NS);
  IcpState* st = S.h<IcpState>(P.st);
  for (size_t i = 0; i < N; ++i) {
    const IcpPair& Q = M.pair[i];
    IcpState& R = st[i];
    for (int e = 0; e < 16; ++e) R.fin[e] = b->guess && e < 12 ? b->guess[16 * (first + i) + e] : (e % 5 == 0 ? 1.0f : 0.0f);
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R.M[3 * r + c] = R.fin[4 * r + c];
      R.t[r] = R.fin[4 * r + 3];
    }
    R.state = BA_ICP_NOT_CONVERGED; R.converged = 0; R.iterations = 0; R.n_corr = 0;
    R.apply_at = 0; R.n_flag = 0;
    R.prev = DBL_MAX; R.fitness = DBL_MAX;
    S.put(P.cur + sizeof(float) * 3 * (size_t)Q.soff, b->xyz + 3 * (size_t)Q.s0, sizeof(float) * 3 * (size_t)Q.ns);
  }
  S.pad(P.st + sizeof(IcpState) * N);
  S.upload(P.xyz);
  S.upload_from(P.xyz, b->xyz, sizeof(float) * 3 * total);
  IcpArgs A{};
  A.n_pair = (int)N; A.max_ns = M.max_ns; A.max_ring = kIcpMaxRing;
  A.max_d2 = icp_gate(p.max_corr_dist); A.fit_range = p.fitness_max_range;
  A.rules = IcpRules{p.max_iterations, p.min_correspondences, p.with_scale, p.mse_abs_eps, p.mse_rel_eps, p.transformation_eps};
  A.pair = S.d<const IcpPair>(P.pair); A.grid = S.d<const IcpGrid>(P.grid);
  A.cell_start = S.d<const int>(P.cell_start); A.sorted = S.d<const IcpPt>(P.sorted);
  A.xyz = S.d<const float>(P.xyz); A.perm = S.d<const int>(P.perm);
  A.st = S.d<IcpState>(P.st); A.cur = S.d<float>(P.cur); A.idx = S.d<int>(P.idx); A.d2 = S.d<float>(P.d2);
  A.flag = S.d<int>(P.flag); A.part = S.d<double>(P.part); A.mse = S.d<double>(P.mse);
  return A;
}

}  // namespace

int ba_icp(ba_ctx* ctx, const ba_icp_batch* b, const ba_icp_options* opt, ba_icp_result* out, double* mse) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_icp: ";
    const ba_icp_options p = check_icp(fn.c_str(), b, opt);
    const size_t N = b->n_pairs;
    if (N == 0) return;
    if (!out) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    StagingArena& S = ctx->icp;
    S.tic();
    const IcpPlan M = icp_plan(fn.c_str(), b, p, 0, (int)N);
    const IcpLayout P = icp_layout(M, (size_t)b->set_offset[b->n_sets], p.max_iterations, false);
    const IcpArgs A = icp_stage(ctx, b, p, M, P, 0, fn);
    HIP_OK(hipMemsetAsync(A.mse, 0, sizeof(double) * N * (size_t)p.max_iterations, ctx->stream));
    S.kernels_begin();
    for (int round = 0; round <= p.max_iterations; ++round) launch_icp_round(A, round, false, ctx->stream);
    S.kernels_end();
    S.fetch(P.st, sizeof(IcpState) * N);   // the states are input and output
    S.download();
    const IcpState* st = S.h<IcpState>(P.st);
    for (size_t i = 0; i < N; ++i) {
      ba_icp_result& R = out[i];
      std::memcpy(R.final, st[i].fin, sizeof R.final);
      R.converged = st[i].converged; R.state = st[i].state; R.iterations = st[i].iterations; R.n_corr = st[i].n_corr;
      R.fitness = st[i].fitness;
    }
    S.copy_out(mse, P.mse, sizeof(double) * N * (size_t)p.max_iterations);
    S.finish({S.kernels_done() / (p.max_iterations + 1)});
  });
}

int ba_icp_nn(ba_ctx* ctx, const ba_icp_batch* b, int pair, const ba_icp_options* opt, int32_t* idx, float* d2) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    const std::string fn = "ba_icp_nn: ";
    const ba_icp_options p = check_icp(fn.c_str(), b, opt);
    if (pair < 0 || pair >= b->n_pairs)
      throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "pair " + std::to_string(pair) + " out of range"};
    if (!idx || !d2) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + "null output array"};
    const IcpPlan M = icp_plan(fn.c_str(), b, p, pair, 1);
    const IcpLayout P = icp_layout(M, (size_t)b->set_offset[b->n_sets], p.max_iterations, true);
    const IcpArgs A = icp_stage(ctx, b, p, M, P, pair, fn);
    launch_icp_round(A, 0, true, ctx->stream);
    ctx->icp.download();
    ctx->icp.copy_out(idx, P.idx, sizeof(int32_t) * M.NS); ctx->icp.copy_out(d2, P.d2, sizeof(float) * M.NS);
  });
}

}  // extern "C"
