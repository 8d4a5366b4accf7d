// ba_solver.hip — host side of libba_hip.so: problem structure, device
// workspace, the Levenberg-Marquardt driver, covariance, the debug entries, the
// communicator and create / destroy of the extern "C" ABI (include/ba_hip.h).
// The context is ba_ctx.h; the batch entry points are ba_batch.hip.
//
// The driver restates ceres::TrustRegionMinimizer + LevenbergMarquardtStrategy
// with the options of BAOptimizer::configureSolver (reference
// ba_project/src/ba/Optimizer.cpp:80-90) and drives the CDNA4 kernels of
// ba_kernels.hip.  Per LM iteration the host reads back one small scalar
// record (cost, model cost change, norms, failure counts) to take Ceres'
// accept / reject / terminate decisions; all vectors stay in HBM.
//
// Multi-GPU: every rank owns a disjoint set of points with all their
// observations; cameras are replicated.  RCCL all-reduces (over xGMI) the
// per-camera blocks after linearisation, the dense reduced camera system
// after point elimination, and the scalar record after the candidate pass.
// All ranks then take identical decisions.
#include <cmath>
#include <cstdio>
#include <limits>
#include <numeric>

#include "ba_ctx.h"
#include "ba_device.h"

using namespace bahip;

namespace {

// hipFree at scope exit (buffers that live for one call)
struct DevFree { void* p; ~DevFree() { (void)hipFree(p); } };

// ---------------------------------------------------------------------------
// structure build
// ---------------------------------------------------------------------------
void set_problem(ba_ctx* ctx, const ba_problem* pb) {
  if (!pb) throw BaError{BA_ERR_INVALID_ARGUMENT, "problem is NULL"};
  const int nc = pb->n_cams, np = pb->n_pts, no = pb->n_obs;
  if (nc < 0 || np < 0 || no < 0) throw BaError{BA_ERR_INVALID_ARGUMENT, "negative size"};
  if ((nc > 0 && (!pb->cams || !pb->K)) || (np > 0 && !pb->pts) ||
      (no > 0 && (!pb->obs_cam || !pb->obs_pt || !pb->obs_uv)))
    throw BaError{BA_ERR_INVALID_ARGUMENT, "missing array"};
  bool any_fixed = false;
  for (int c = 0; c < nc; ++c) any_fixed |= (pb->cam_fixed && pb->cam_fixed[c]);
  if (any_fixed && !pb->cam_fixed_extr) throw BaError{BA_ERR_INVALID_ARGUMENT, "cam_fixed_extr required for fixed cameras"};
  for (int o = 0; o < no; ++o) {
    if (pb->obs_cam[o] < 0 || pb->obs_cam[o] >= nc || pb->obs_pt[o] < 0 || pb->obs_pt[o] >= np)
      throw BaError{BA_ERR_INVALID_ARGUMENT, "observation index out of range at obs " + std::to_string(o)};
  }
  ctx->free_problem();
  HIP_OK(hipSetDevice(ctx->device));
  ctx->nc = nc; ctx->np = np; ctx->no = no;
  ctx->huber_a = pb->huber_a;
  ctx->cam_fixed_h.assign(nc, 0);
  for (int c = 0; c < nc; ++c) ctx->cam_fixed_h[c] = pb->cam_fixed ? pb->cam_fixed[c] : 0;
  std::vector<uint8_t> pt_fixed(np, 0);
  for (int p = 0; p < np; ++p) pt_fixed[p] = pb->pt_fixed ? pb->pt_fixed[p] : 0;

  // sort observations by (point, camera, caller index): counting sort by point
  std::vector<int> pt_off(np + 1, 0);
  for (int o = 0; o < no; ++o) pt_off[pb->obs_pt[o] + 1]++;
  for (int p = 0; p < np; ++p) pt_off[p + 1] += pt_off[p];
  std::vector<int> perm(no);
  {
    std::vector<int> fill(pt_off.begin(), pt_off.end() - 1);
    for (int o = 0; o < no; ++o) perm[fill[pb->obs_pt[o]]++] = o;
    for (int p = 0; p < np; ++p) {
      auto b = perm.begin() + pt_off[p], e = perm.begin() + pt_off[p + 1];
      if (e - b > 1)
        std::stable_sort(b, e, [&](int a, int c) { return pb->obs_cam[a] < pb->obs_cam[c]; });
    }
  }
  // active blocks
  std::vector<int> vc(nc, -1);
  std::vector<uint8_t> pt_var(np, 0), cam_used(nc, 0);
  for (int o = 0; o < no; ++o) {
    const int c = pb->obs_cam[o], p = pb->obs_pt[o];
    if (!ctx->cam_fixed_h[c]) cam_used[c] = 1;
    if (!pt_fixed[p]) pt_var[p] = 1;
  }
  if (ctx->coll() && nc > 0) {
    // the reduced system spans the union of the ranks' observed cameras
    std::vector<double> u(nc);
    for (int c = 0; c < nc; ++c) u[c] = cam_used[c];
    ctx->allreduce_host_values(u.data(), nc, 1);
    for (int c = 0; c < nc; ++c) cam_used[c] = u[c] != 0.0;
  }
  ctx->max_no = no;
  if (ctx->coll()) {
    // every rank takes the same matvec path (ITERATIVE_SCHUR), chosen from the
    // largest shard: identical kernels and rounding on every rank
    double h = (double)no;
    ctx->allreduce_host_values(&h, 1, 1);
    ctx->max_no = (int)h;
  }
  ctx->cam_of_vc.clear();
  for (int c = 0; c < nc; ++c)
    if (cam_used[c]) { vc[c] = (int)ctx->cam_of_vc.size(); ctx->cam_of_vc.push_back(c); }
  const int nvc = (int)ctx->cam_of_vc.size();
  ctx->nvc = nvc;
  ctx->n = 6 * nvc;
  ctx->ld = ctx->n;

  std::vector<int> obs_cam(no), obs_pt(no);
  std::vector<float2> uv(no);
  for (int s = 0; s < no; ++s) {
    const int o = perm[s];
    obs_cam[s] = pb->obs_cam[o];
    obs_pt[s] = pb->obs_pt[o];
    uv[s] = make_float2(pb->obs_uv[2 * o], pb->obs_uv[2 * o + 1]);
  }
  // observations by variable camera (increasing sorted index)
  std::vector<int> cam_off(nvc + 1, 0);
  for (int s = 0; s < no; ++s) if (vc[obs_cam[s]] >= 0) cam_off[vc[obs_cam[s]] + 1]++;
  for (int v = 0; v < nvc; ++v) cam_off[v + 1] += cam_off[v];
  std::vector<int> cam_obs(cam_off[nvc]);
  {
    std::vector<int> fill(cam_off.begin(), cam_off.end() - 1);
    for (int s = 0; s < no; ++s) if (vc[obs_cam[s]] >= 0) cam_obs[fill[vc[obs_cam[s]]]++] = s;
  }
  // ---- device upload
  DevProblem& P = ctx->P;
  P = DevProblem{};
  P.nc = nc; P.np = np; P.no = no; P.nvc = nvc; P.n = ctx->n; P.ld = ctx->ld;
  P.huber_a = pb->huber_a;
  P.huber_b = pb->huber_a * pb->huber_a;
  P.obs_cam = ctx->upload(obs_cam);
  P.obs_pt = ctx->upload(obs_pt);
  P.uv = ctx->upload(uv);
  P.pt_off = ctx->upload(pt_off);
  P.cam_off = ctx->upload(cam_off);
  {
    std::vector<int2> cam_op(cam_obs.size());
    for (size_t i = 0; i < cam_obs.size(); ++i) cam_op[i] = make_int2(cam_obs[i], obs_pt[cam_obs[i]]);
    P.cam_op = ctx->upload(cam_op);
    std::vector<float2> uv_cm(cam_obs.size());
    for (size_t i = 0; i < cam_obs.size(); ++i) uv_cm[i] = uv[cam_obs[i]];
    P.uv_cm = ctx->upload(uv_cm);
  }
  P.vc = ctx->upload(vc);
  {
    std::vector<int> obs_vc(no);
    for (int o = 0; o < no; ++o) obs_vc[o] = vc[obs_cam[o]];
    P.obs_vc = ctx->upload(obs_vc);
  }
  P.cam_of_vc = ctx->upload(ctx->cam_of_vc);
  P.cam_fixed = ctx->upload(ctx->cam_fixed_h);
  P.pt_var = ctx->upload(pt_var);
  P.K = ctx->upload(std::vector<float>(pb->K, pb->K + 9 * (size_t)nc));
  ctx->k_plain = true;   // no skew, row 2 = (0, 0, k22): the 16-value PCG records apply
  for (int c = 0; c < nc; ++c) {
    const float* k = pb->K + 9 * (size_t)c;   // column-major
    if (k[1] != 0.0f || k[2] != 0.0f || k[3] != 0.0f || k[5] != 0.0f) ctx->k_plain = false;
  }
  {
    std::vector<float> ex(16 * (size_t)nc, 0.0f);
    if (pb->cam_fixed_extr)
      for (int c = 0; c < nc; ++c)
        if (ctx->cam_fixed_h[c]) std::memcpy(&ex[16 * (size_t)c], pb->cam_fixed_extr + 16 * (size_t)c, 16 * sizeof(float));
    P.extr = ctx->upload(ex);
  }
  DevWork& W = ctx->W;
  W = DevWork{};
  W.cams = ctx->upload(std::vector<double>(pb->cams, pb->cams + 6 * (size_t)nc));
  W.pts = ctx->upload(std::vector<double>(pb->pts, pb->pts + 3 * (size_t)np));
  W.cams_c = ctx->dalloc<double>(6 * (size_t)nc);
  W.pts_c = ctx->dalloc<double>(3 * (size_t)np);
  W.rec = ctx->dalloc<double>((size_t)kCamRec * nc);
  W.rec_c = ctx->dalloc<double>((size_t)kCamRec * nc);
  W.crec = ctx->dalloc<double>((size_t)16 * nc);
  W.ctbl = ctx->dalloc<double>((size_t)22 * nc);
  // J-free iteration: r and J are recomputed by every consumer and never
  // stored (camera tables in LDS up to 200 cameras, the compact 128-B camera
  // records beyond: each observation forms its camera's dual Rodrigues from
  // them); BA_JR=1 forces the JR-materialising kernels (A/B,
  // diagnostics).  JR is then allocated only for ba_linearize's read-back.
  {
    const char* e = std::getenv("BA_JR");
    W.jrfree = nc > 0 && !(e && e[0] == '1');
  }
  W.JR = W.jrfree ? nullptr : ctx->dalloc<double>((size_t)(bahip::jr_ja_host(nc) + 8) * no);   // JA [no][jr_ja] + JB [no][8] (ba_kernels.hip)
  W.delta_p = ctx->dalloc<double>(3 * (size_t)np);
  W.pxv = ctx->dalloc<double>(4 * (size_t)np);
  W.Hpp = ctx->dalloc<double>(6 * (size_t)np);
  W.gp = ctx->dalloc<double>(3 * (size_t)np);
  W.scale_p = ctx->dalloc<double>(3 * (size_t)np);
  W.diag_p = ctx->dalloc<double>(3 * (size_t)np);
  W.Linv = ctx->dalloc<double>(6 * (size_t)np);
  W.u = ctx->dalloc<double>(4 * (size_t)np);
  // Hcc | gc | scalar slots | PCG state in one allocation: the camera blocks
  // and the point-side sums cross ranks in one all-reduce
  {
    double* hx = ctx->dalloc<double>(27 * (size_t)nvc + kNumSlots + kPcgState);
    W.Hcc = hx;
    W.gc = hx + 21 * (size_t)nvc;
    W.scal = hx + 27 * (size_t)nvc;
  }
  W.scale_c = ctx->dalloc<double>(6 * (size_t)nvc);
  W.diag_c = ctx->dalloc<double>(6 * (size_t)nvc);
  W.delta_c = ctx->dalloc<double>(6 * (size_t)nvc);
  W.W = nullptr;   // per-observation Schur blocks: allocated by the first solve (fp64 or fp32)
  W.Wf = nullptr;
  W.y = ctx->dalloc<double>(std::max(ctx->n, 1));
  W.part = ctx->dalloc<double>((size_t)kNumSlots * kMaxBlocks);
  W.cam_split = nvc > 0 ? std::min(kCamSplit, std::max(1, 2048 / nvc)) : 1;
  W.cpart = ctx->dalloc<double>((size_t)W.cam_split * 27 * std::max(nvc, 1));

  HIP_OK(hipMemsetAsync(W.part, 0, sizeof(double) * kNumSlots * kMaxBlocks, ctx->stream));
  HIP_OK(hipMemsetAsync(W.scal, 0, sizeof(double) * (kNumSlots + kPcgState), ctx->stream));
  HIP_OK(hipStreamSynchronize(ctx->stream));
  ctx->perm.swap(perm);
  ctx->h_pt_off.swap(pt_off);
  ctx->h_obs_cam.swap(obs_cam);
  ctx->h_vc.swap(vc);
  ctx->h_pt_var.swap(pt_var);
  ctx->pt_fixed_h.swap(pt_fixed);
  ctx->have_problem = true;
}

// The overlapped form's plan (ba_kernels.h OvPlan, ba_chol_persist.hip
// OvArgs): every S entry of the lower tiles is rewritten each step (no empty
// camera pair, no point observed twice by one camera), the persistent grid
// fits, and the launch takes every CU.  Work items per XCD queue in tile-column
// order: for each tile column, the diagonal slices of its cameras (dealt
// round-robin over the queues), then its pair blocks in row-major order, cut
// into 8 contiguous runs of equal pair count (one per queue: the runs of a
// column are formed side by side) and grouped 4 to an item.
void build_overlap_plan(ba_ctx* ctx, const std::vector<int4>& blocks) {
  DevWork& W = ctx->W;
  W.ov = OvPlan{};
  const int n = ctx->n, nvc = ctx->nvc, G = W.cam_split;
  const int T = (n + 63) / 64, TR = (n + 1 + 63) / 64;
  if (!W.chol_persist || nvc == 0 || nvc > bahip::kLinLdsCamsHost || ctx->dup_diag || W.s_memset || W.neblocks != 0)
    return;
  const int cap = bahip::chol_persist_capacity(ctx->device);
  int grid = 1;
  for (int j = 1; j < T; ++j) grid += TR - (j == 1 ? 2 : j);   // (chol_persist_grid)
  // (at least one helper per XCD queue: a queue's last items are then always
  // taken, whatever the workers are waiting for)
  if (cap < grid + 8) return;
  grid = cap;
  std::vector<unsigned> tgt((size_t)TR * T, 0);
  auto tile = [&](int r, int c) { return (size_t)(r >> 6) * T + (c >> 6); };
  std::vector<std::vector<int>> colblk(T);
  for (size_t b = 0; b < blocks.size(); ++b) {
    const int I = blocks[b].x, J = blocks[b].y;
    if (I <= J) return;   // (a diagonal pair block: not this form)
    colblk[(6 * J) >> 6].push_back((int)b);
    const int r0 = 6 * I, c0 = 6 * J;
    std::vector<size_t> ts = {tile(r0, c0), tile(r0, c0 + 5), tile(r0 + 5, c0), tile(r0 + 5, c0 + 5)};
    std::sort(ts.begin(), ts.end());
    ts.erase(std::unique(ts.begin(), ts.end()), ts.end());
    for (size_t t : ts) ++tgt[t];
  }
  for (int v = 0; v < nvc; ++v)
    for (int k = 0; k < 27; ++k) {
      int row, col;
      if (k < 21) {
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= k) ++a;
        row = 6 * v + a;
        col = 6 * v + k - a * (a + 1) / 2;
      } else {
        row = n;
        col = 6 * v + k - 21;
      }
      ++tgt[tile(row, col)];
    }
  for (int I = 0; I < TR; ++I)
    for (int J = 0; J < T && J <= I; ++J)
      if (tgt[(size_t)I * T + J] == 0) return;   // (a lower tile nothing writes)
  std::vector<int4> items[8];   // four records to an item
  int unit_rr = 0;
  for (int tc = 0; tc < T; ++tc) {
    for (int v = 0; v < nvc; ++v) {
      if ((6 * v) >> 6 != tc) continue;
      for (int g = 0; g < G; ++g) {
        const int x = unit_rr++ & 7;
        items[x].push_back(make_int4(-1 - (v * G + g), 0, 0, 0));
        for (int q = 1; q < 4; ++q) items[x].push_back(make_int4(0, 0, 0, 0));
      }
    }
    const std::vector<int>& cb = colblk[tc];
    long long tot = 0;
    for (int b : cb) tot += blocks[b].w - blocks[b].z;
    size_t k = 0;
    long long acc = 0;
    for (int x = 0; x < 8; ++x) {
      const long long until = tot * (x + 1) / 8;
      std::vector<int> run;
      while (k < cb.size() && (acc < until || x == 7)) {
        acc += blocks[cb[k]].w - blocks[cb[k]].z;
        run.push_back(cb[k++]);
      }
      // four pair blocks to an item.  (Measured and not kept: one block to an
      // item in the first columns, to start the chain sooner — C3 0.64 to
      // 0.97 ms vs 0.58: an item's fixed cost outweighs its length;
      // profiles/r06_v11_ov_first_cols_ab.txt.)
      for (size_t r = 0; r < run.size(); r += 4)
        for (int q = 0; q < 4; ++q) items[x].push_back(r + q < run.size() ? blocks[run[r + q]] : make_int4(0, 0, 0, 0));
    }
  }
  std::vector<int4> all;
  OvPlan& P = W.ov;
  for (int x = 0; x < 8; ++x) {
    P.ioff[x] = (int)(all.size() / 4);
    all.insert(all.end(), items[x].begin(), items[x].end());
  }
  P.ioff[8] = (int)(all.size() / 4);
  P.irec = ctx->upload(all);
  P.tgt = ctx->upload(tgt);
  const size_t nctr = 2 * (size_t)TR * T + nvc + 8;   // cnt | cam_cnt | q | pflag
  P.ctr = ctx->dalloc<unsigned>(nctr);
  HIP_OK(hipMemsetAsync(P.ctr, 0, sizeof(unsigned) * nctr, ctx->stream));
  P.grid = grid;
  P.launches = 0;
  P.ok = true;
}

// DENSE_SCHUR structures (built on the first dense solve): the dense reduced
// system S / factor Lf (16 n^2 bytes), Cholesky block inverses, and the Schur
// pair lists.
void ensure_dense(ba_ctx* ctx) {
  if (ctx->have_dense) return;
  const int np = ctx->np, nvc = ctx->nvc;
  const std::vector<int>& pt_off = ctx->h_pt_off;
  const std::vector<int>& obs_cam = ctx->h_obs_cam;
  const std::vector<int>& vc = ctx->h_vc;
  const std::vector<uint8_t>& pt_var = ctx->h_pt_var;
  // Schur pair lists: for every variable point, every pair of its observations
  // by variable cameras contributes W_a W_b^T to block (vc_a, vc_b), vc_a >= vc_b.
  std::vector<int4> blocks;
  std::vector<int2> pairs;
  {
    struct PE { int64_t key; int a, b; };
    std::vector<PE> pe;
    size_t est = 0;
    for (int p = 0; p < np; ++p) if (pt_var[p]) { const size_t k = pt_off[p + 1] - pt_off[p]; est += k * (k - 1) / 2; }
    pe.reserve(est);
    std::vector<int> lst;
    for (int p = 0; p < np; ++p) {
      if (!pt_var[p]) continue;
      lst.clear();
      for (int s = pt_off[p]; s < pt_off[p + 1]; ++s) if (vc[obs_cam[s]] >= 0) lst.push_back(s);
      for (size_t i = 0; i < lst.size(); ++i)
        for (size_t j = 0; j < i; ++j) {
          const int a = lst[i], b = lst[j];        // vc[a] >= vc[b] (sorted by camera)
          const int I = vc[obs_cam[a]], J = vc[obs_cam[b]];
          const int64_t key = (int64_t)I * nvc + J;
          pe.push_back({key, a, b});
          if (I == J) pe.push_back({key, b, a});    // duplicate camera on one point
        }
    }
    // stable counting/radix by key keeps point order inside a block
    std::stable_sort(pe.begin(), pe.end(), [](const PE& x, const PE& y) { return x.key < y.key; });
    pairs.resize(pe.size());
    for (size_t i = 0; i < pe.size(); ++i) {
      pairs[i] = make_int2(pe[i].a, pe[i].b);
      if (i == 0 || pe[i].key != pe[i - 1].key) {
        if (!blocks.empty()) blocks.back().w = (int)i;
        blocks.push_back(make_int4((int)(pe[i].key / nvc), (int)(pe[i].key % nvc), (int)i, 0));
      }
    }
    if (!blocks.empty()) blocks.back().w = (int)pe.size();
  }
  {
    const int T = (ctx->n + 63) / 64, cap = bahip::back_flow_capacity(ctx->device);
    if (cap < 0) throw BaError{BA_ERR_DEVICE, "occupancy query for the back substitution failed"};
    if (T > cap)
      throw BaError{BA_ERR_INVALID_ARGUMENT, "DENSE_SCHUR: " + std::to_string(T) + " block columns exceed the " +
                                                 std::to_string(cap) + " resident back-substitution workgroups; "
                                                 "use ITERATIVE_SCHUR"};
  }
  DevWork& W = ctx->W;
  W.S = ctx->dalloc<double>((size_t)(ctx->n + 1) * std::max(ctx->ld, 1));
  W.Lf = ctx->dalloc<double>((size_t)(ctx->n + 1) * std::max(ctx->ld, 1));
  const bool split = (ctx->n + 63) / 64 >= bahip::chol_split_blocks();
  W.Ubuf = split ? nullptr : ctx->dalloc<double>((size_t)(ctx->n + 1) * std::max(ctx->ld, 1));
  W.Vbuf = ctx->dalloc<double>((size_t)((ctx->n + 63) / 64 + 1) * 64 * 64);
  W.ctask = nullptr;
  W.ctask_off = nullptr;
  std::vector<int4> tasks_h;
  if (split) {
    bahip::chol_split_tasks(ctx->n, tasks_h, ctx->chol_off);
    W.ctask = ctx->upload(tasks_h);
    W.ctask_off = ctx->chol_off.data();
  }
  W.chol_fuse = W.ctask && bahip::chol_split_fused();
  W.chol_flow = false;
  W.ftask = nullptr;
  W.nftask = 0;
  W.tflag = nullptr;
  if (W.ctask && bahip::chol_split_flow() &&
      (size_t)(ctx->n + 1) * std::max(ctx->ld, 1) * sizeof(double) < ((size_t)1 << 31)) {   // (32-bit buffer offsets)
    std::vector<int4> flow;
    bahip::chol_flow_tasks(tasks_h, ctx->chol_off, flow);
    W.ftask = ctx->upload(flow);
    W.nftask = (int)flow.size();
    const size_t T = (ctx->n + 63) / 64, TR = (ctx->n + 1 + 63) / 64;
    W.tflag = ctx->dalloc<unsigned>(2 * TR * T);
    HIP_OK(hipMemsetAsync(W.tflag, 0, sizeof(unsigned) * 2 * TR * T, ctx->stream));
    W.chol_flow = true;
  }
  W.yg = ctx->dalloc<double>(2 * (size_t)std::max(ctx->n, 1));
  {
    // persistent factorisation (one launch) when the per-step form would not
    // split and the whole grid is resident; BA_CHOL_PERSIST=0 forces the
    // per-step launches (A/B).  Not with the host-staged transport: its ranks
    // may share one GPU, and their persistent grids need not all fit at once
    // (a spin bound would then be hit on some ranks only, and the ranks'
    // steps would diverge)
    const int T = (ctx->n + 63) / 64, TR = (ctx->n + 1 + 63) / 64;
    const char* env = std::getenv("BA_CHOL_PERSIST");
    W.chol_persist = ctx->n > 0 && T < bahip::chol_split_blocks() && !(env && env[0] == '0') && !ctx->host_fn &&
                     bahip::chol_persist_fits(ctx->device, ctx->n);
    const size_t nf = (size_t)T + (size_t)TR * T;
    W.cflags = ctx->dalloc<unsigned>(nf);
    HIP_OK(hipMemsetAsync(W.cflags, 0, sizeof(unsigned) * std::max<size_t>(nf, 1), ctx->stream));
  }
  W.Spk = nullptr;
  // diagonal pair blocks (a point observed twice by one camera) update the
  // S diagonal after the fold: the LM diagonal is then added after them
  // (separate k_cam_add_diag), in the order the exchange path uses
  ctx->dup_diag = std::any_of(blocks.begin(), blocks.end(), [](const int4& b) { return b.x == b.y; });
  // k_schur_pairs*: XCD x sweeps the blocks [xoff[x], xoff[x+1]): equal
  // contiguous ranges of the row-major list (bands of rows: C3 165 vs 188 us
  // for an interleave)
  std::vector<int> xoff(9, 0);
  {
    const int R = ((int)blocks.size() + 7) / 8;
    for (int x = 0; x <= 8; ++x) xoff[x] = std::min((int)blocks.size(), x * R);
    W.xmax = R;
  }
  W.blocks = ctx->upload(blocks);
  W.nblocks = (int)blocks.size();
  W.xoff = ctx->upload(xoff);
  W.pairs = ctx->upload(pairs);
  HIP_OK(hipMemsetAsync(W.yg, 0, sizeof(double) * 2 * (size_t)std::max(ctx->n, 1), ctx->stream));
  // S is rewritten every step (diagonal blocks, rhs and every co-observed
  // block); the rest of the lower triangle must be re-zeroed (the Cholesky
  // updates it in place): a list of those blocks, or a memset when they are
  // the majority
  {
    const size_t nlow = (size_t)nvc * (nvc - (nvc > 0 ? 1 : 0)) / 2;
    const size_t nfull = (size_t)std::count_if(blocks.begin(), blocks.end(), [](const int4& b) { return b.x != b.y; });
    const size_t nempty = nlow - nfull;
    W.s_memset = nempty > nfull || nempty > (size_t)(1 << 22);
    W.neblocks = 0;
    W.eblocks = nullptr;
    if (!W.s_memset && nempty > 0) {
      std::vector<uint8_t> used(nlow, 0);
      auto lid = [](size_t I, size_t J) { return I * (I - 1) / 2 + J; };   // I > J
      for (const int4& b : blocks) if (b.x != b.y) used[lid(b.x, b.y)] = 1;
      std::vector<int2> eb;
      eb.reserve(nempty);
      for (int I = 1; I < nvc; ++I)
        for (int J = 0; J < I; ++J) if (!used[lid(I, J)]) eb.push_back(make_int2(I, J));
      W.eblocks = ctx->upload(eb);
      W.neblocks = (int)eb.size();
    }
  }
  HIP_OK(hipMemsetAsync(W.S, 0, sizeof(double) * (size_t)(ctx->n + 1) * std::max(ctx->ld, 1), ctx->stream));
  build_overlap_plan(ctx, blocks);
  HIP_OK(hipStreamSynchronize(ctx->stream));
  ctx->have_dense = true;
}

// ITERATIVE_SCHUR structures: compact diagonal blocks, preconditioner, CG
// vectors, matvec scratch, and the (rare) pairs of observations of one point
// by one camera, whose cross terms belong to the Schur-Jacobi diagonal block.
void ensure_pcg(ba_ctx* ctx) {
  if (ctx->have_pcg) return;
  const int np = ctx->np, nvc = ctx->nvc;
  const size_t n = (size_t)std::max(ctx->n, 1);
  DevWork& W = ctx->W;
  W.pcg_G = W.cam_split;
  W.Sd = ctx->dalloc<double>(27 * (size_t)std::max(nvc, 1));
  W.Adiag = ctx->dalloc<double>(21 * (size_t)std::max(nvc, 1));
  W.Minv = ctx->dalloc<double>(36 * (size_t)std::max(nvc, 1));
  W.pb = ctx->dalloc<double>(n);
  W.pr = ctx->dalloc<double>(n);
  W.pz = ctx->dalloc<double>(n);
  W.pp = ctx->dalloc<double>(n);
  W.pq = ctx->dalloc<double>(n);
  W.vpt = ctx->dalloc<double>(3 * (size_t)std::max(np, 1));
  W.vacc = ctx->dalloc<double>(3 * (size_t)std::max(np, 1));
  // a point with no observation never gets a vpt entry (the point passes
  // store it at the end of a point's run), but k_pcg_vacc folds every point:
  // zeros, so such a point's accumulated product and step stay 0
  HIP_OK(hipMemsetAsync(W.vpt, 0, sizeof(double) * 3 * (size_t)std::max(np, 1), ctx->stream));
  HIP_OK(hipMemsetAsync(W.vacc, 0, sizeof(double) * 3 * (size_t)std::max(np, 1), ctx->stream));
  W.tpart = ctx->dalloc<double>((size_t)W.pcg_G * 6 * std::max(nvc, 1));
  W.ppart = ctx->dalloc<double>(3 * (size_t)kMaxBlocks);
  if ((nvc + 255) / 256 > kMaxBlocks) throw BaError{BA_ERR_INVALID_ARGUMENT, "too many cameras for ITERATIVE_SCHUR"};
  std::vector<int> dup_off(nvc + 1, 0);
  std::vector<int2> dup;
  {
    std::vector<std::vector<int2>> per(nvc);
    for (int p = 0; p < np; ++p) {
      if (!ctx->h_pt_var[p]) continue;
      for (int a = ctx->h_pt_off[p]; a < ctx->h_pt_off[p + 1]; ++a)
        for (int b = a + 1; b < ctx->h_pt_off[p + 1] && ctx->h_obs_cam[b] == ctx->h_obs_cam[a]; ++b) {
          const int v = ctx->h_vc[ctx->h_obs_cam[a]];
          if (v >= 0) per[v].push_back(make_int2(a, b));
        }
    }
    for (int v = 0; v < nvc; ++v) {
      dup_off[v + 1] = dup_off[v] + (int)per[v].size();
      dup.insert(dup.end(), per[v].begin(), per[v].end());
    }
  }
  W.dup_off = ctx->upload(dup_off);
  W.dup_pairs = ctx->upload(dup);
  ctx->pcg_ndup = dup.size();
  {
    // point-aligned chunks of <= 64 observations for the PCG point pass
    // (k_pcg_point_seg); BA_PCG_SEG=0 keeps the value-pair passes
    const char* e = std::getenv("BA_PCG_SEG");
    std::vector<int2> ch;
    bool ok = !(e && e[0] == '0');
    int start = 0;
    for (int p = 0; p < np && ok; ++p) {
      const int a = ctx->h_pt_off[p], b = ctx->h_pt_off[p + 1];
      if (b - a > 64) { ok = false; break; }
      if (b - start > 64) { ch.push_back(make_int2(start, a)); start = a; }
    }
    if (ok && ctx->no > start) ch.push_back(make_int2(start, ctx->no));
    W.npchunks = ok ? (int)ch.size() : 0;
    W.pchunks = ok && !ch.empty() ? ctx->upload(ch) : nullptr;
    if (!W.pchunks) W.npchunks = 0;
  }
  HIP_OK(hipStreamSynchronize(ctx->stream));
  ctx->have_pcg = true;
}

// ---------------------------------------------------------------------------
// LM phases
// ---------------------------------------------------------------------------
struct LinResult { double cost, gmax, gnorm, xnorm; bool ok; };

constexpr uint32_t bit(int s) { return 1u << s; }

// Linearisation phase: enqueue (no host sync) / read back.  The solver
// enqueues the next trust-region step right behind an accepted step's
// linearisation and reads both records with one host sync (the step is
// wasted only when the new gradient ends the solve).
// defer_reduce: a step_enqueue follows before the next read_scalars and
// folds this linearisation's scalars with its own (single rank only)
void linearize_enqueue(ba_ctx* ctx, bool compute_scale, double min_diag, double max_diag, bool time_rj = false,
                       bool defer_reduce = false) {
  const hipStream_t s = ctx->stream;
  DevProblem& P = ctx->P;
  DevWork& W = ctx->W;
  ctx->lin_at_cand = false;
  launch_lin_prep(P, W, s);
  // time_rj: kernel execution stamps from the launch itself (bench roofline),
  // into the stamp pair ctx->rj_slot
  hipEvent_t e0 = time_rj ? ctx->ev[2 + 2 * ctx->rj_slot] : nullptr, e1 = time_rj ? ctx->ev[3 + 2 * ctx->rj_slot] : nullptr;
  launch_linearize(P, W, s, e0, e1);
  // (J-free: the timed residual + Jacobian kernel is k_lin_point, launched here)
  launch_point_assemble(P, W, compute_scale, min_diag, max_diag, s, W.jrfree ? e0 : nullptr, W.jrfree ? e1 : nullptr);
  launch_cam_assemble(P, W, s);
  // point-side scalars: folded here when they must be all-reduced before
  // cam_norms, else together with the camera-side ones (one launch less)
  const uint32_t lin_sum = bit(SL_COST) | bit(SL_LIN_BAD) | bit(SL_GN2_P) | bit(SL_XN2_P);
  if (ctx->coll()) launch_reduce(W, lin_sum, bit(SL_GMAX_P), s);
  if (ctx->coll()) {
    // Hcc, gc, COST, LIN_BAD, GN2_P, XN2_P (contiguous), then the max
    ctx->allreduce(W.Hcc, 27 * (size_t)ctx->nvc + SL_GMAX_P);
    ctx->allreduce(W.scal + SL_GMAX_P, 1, ncclMax);
  }
  // deferred fold (single rank): the norms ride in the step's point
  // elimination (BA_NORMS_FOLD=0: their own launch here)
  const char* nfe = getenv("BA_NORMS_FOLD");   // (read per call: tests switch it)
  const bool norms_fold_on = !(nfe && nfe[0] == '0');
  if (defer_reduce && !ctx->coll() && norms_fold_on) {
    ctx->norms_pend = true;
    ctx->norms_args = norms_fold(W, compute_scale, min_diag, max_diag);
  } else {
    ctx->norms_pend = false;
    launch_cam_norms(P, W, compute_scale, min_diag, max_diag, s);
  }
  const uint32_t sum_mask = bit(SL_GN2_C) | bit(SL_XN2_C) | (ctx->coll() ? 0u : lin_sum);
  const uint32_t max_mask = bit(SL_GMAX_C) | (ctx->coll() ? 0u : bit(SL_GMAX_P));
  if (defer_reduce && !ctx->coll()) {
    ctx->pend_sum |= sum_mask;
    ctx->pend_max |= max_mask;
  } else {
    launch_reduce(W, sum_mask, max_mask, s);
  }
  if (compute_scale) ctx->scale_valid = true;
}

// after ctx->read_scalars()
LinResult lin_result(ba_ctx* ctx) {
  const double* h = ctx->h_scal;
  LinResult r;
  r.cost = h[SL_COST];
  r.gmax = std::max(h[SL_GMAX_P], h[SL_GMAX_C]);
  r.gnorm = std::sqrt(h[SL_GN2_P] + h[SL_GN2_C]);
  r.xnorm = std::sqrt(h[SL_XN2_P] + h[SL_XN2_C]);
  r.ok = h[SL_LIN_BAD] == 0.0 && std::isfinite(r.cost);
  return r;
}

LinResult linearize(ba_ctx* ctx, bool compute_scale, double min_diag, double max_diag) {
  // a fresh start (solve / bench entry): folds still pending belong to work
  // an earlier call abandoned (e.g. the speculative linearisation behind a
  // solve's last step) and must not be folded into this record
  ctx->clear_pending();
  linearize_enqueue(ctx, compute_scale, min_diag, max_diag);
  ctx->read_scalars();
  return lin_result(ctx);
}

struct StepResult { bool linear_ok; double mcc, cand_cost, step_norm; int ls_iters; bool spin; };

// DENSE_SCHUR: explicit reduced camera system (form_reduced_dense) + dense
// Cholesky
// Returns true when S is left to the factorisation's launch (the overlapped
// form, launch_cholesky_solve_ov: single rank, compact W records, the
// persistent factorisation; BA_CHOL_OVERLAP=0, read per step, or
// allow_ov = false keeps the separate pair / diagonal / fold launches)
bool form_reduced_dense(ba_ctx* ctx, double radius, bool allow_ov = true) {
  const hipStream_t s = ctx->stream;
  DevProblem& P = ctx->P;
  DevWork& W = ctx->W;
  ensure_dense(ctx);
  const char* oe = getenv("BA_CHOL_OVERLAP");
  const bool ov = allow_ov && !(oe && oe[0] == '0') && W.ov.ok && W.chol_persist && !ctx->coll() && !ctx->dup_diag &&
                  radius > 0.0 && W.wcompact && !W.jdiag && !W.w32 && ctx->n > 0;
  if (ov) {
    launch_point_elim(P, W, radius, s, ctx->take_norms());
    return true;
  }
  if (ctx->n > 0) {
    if (W.s_memset) HIP_OK(hipMemsetAsync(W.S, 0, sizeof(double) * (size_t)(ctx->n + 1) * ctx->ld, s));
    else launch_zero_blocks(P, W, s);
  }
  launch_point_elim(P, W, radius, s, ctx->take_norms());
  // single rank, no diagonal pair blocks: the LM diagonal goes in with the
  // fold (same operation order as the exchange path's, bitwise)
  const bool fused_diag = !ctx->coll() && !ctx->dup_diag;
  // ... and that fold rides in the pair pass's launch when it can (one
  // launch fewer; the fold writes only the diagonal blocks and the rhs)
  const bool fold_in_pairs = fused_diag && radius > 0.0 && pairs_take_fold(P, W);
  if ((fold_in_pairs && pairs_take_diag(P, W)) || (fused_diag && radius > 0.0 && pairs_take_diag_nt(P, W))) {
    // ... or rather the diagonal slices ride in it (dispatched after the pair
    // workgroups, they fill the pass's tail) and the fold follows
    launch_schur_pairs(P, W, s, 0.0, true);
    launch_cam_fold_diag(P, W, radius, s);
  } else {
    launch_cam_schur_diag(P, W, s, nullptr, fused_diag ? radius : 0.0, fold_in_pairs);
    launch_schur_pairs(P, W, s, fold_in_pairs ? radius : 0.0);
  }
  if (ctx->coll()) launch_reduce(W, bit(SL_ELIM_BAD), 0, s);   // else folded with the step scalars
  if (ctx->coll()) {
    // only the lower triangle and the rhs row of S carry data: all-reduce
    // them packed (n(n+1)/2 + n doubles instead of (n+1) n)
    // (+1: the elimination-failure count rides along)
    const size_t npk = (size_t)ctx->n * (ctx->n + 1) / 2 + ctx->n;
    if (!W.Spk) W.Spk = ctx->dalloc<double>(npk + 1);
    launch_pack_lower(P, W, true, s);
    ctx->allreduce(W.Spk, npk + 1);
    launch_pack_lower(P, W, false, s);
  }
  if (!fused_diag) launch_cam_add_diag(P, W, radius, s);   // (after the exchange)
  return false;
}
void reduced_solve_dense(ba_ctx* ctx, double radius) {
  if (form_reduced_dense(ctx, radius))
    launch_cholesky_solve_ov(ctx->P, ctx->W, ctx->W.ov, radius, ++ctx->chol_epoch, ctx->stream);
  else
    launch_cholesky_solve2(ctx->P, ctx->W, ++ctx->chol_epoch, ctx->stream);
}

// ITERATIVE_SCHUR: implicit Schur complement + PCG (ba_pcg.hip).  The host
// enqueues CG iterations in batches and reads the device-side state record
// between batches (the kernels of iterations past termination return at
// once); every rank enqueues the same sequence, so the RCCL all-reduce of
// each matvec's camera slices stays matched.  Returns the CG iteration count.
int reduced_solve_pcg(ba_ctx* ctx, double radius, const ba_options& o) {
  const hipStream_t s = ctx->stream;
  DevProblem& P = ctx->P;
  DevWork& W = ctx->W;
  ensure_pcg(ctx);
  {
    // per-observation products t_o = W_o v_p: the camera pass then reads 48 B
    // per observation instead of gathering 144 + 24 B.  With the point-aligned
    // chunks (k_pcg_point_seg forms t_o from the W it has just staged, the
    // camera pass gathers them by LDS-DMA) always: C4 shard 1998-2029 ->
    // 2091-2098 M-obs/s (profiles/r04_v13_ab_pcg_t_c4shard.txt).  Without
    // them (k_pcg_point_t re-reads W) only when the fp64 W outgrows the
    // 256-MiB Infinity Cache (C5 shard +2.7 %; below it the extra pass lost
    // ~0.7 %).  BA_PCG_T=0 / 1 (diagnostics) forces it off / on.
    const char* fe = getenv("BA_PCG_T");   // (read per solve: tests switch it)
    const int force = fe ? atoi(fe) : -1;
    // (the Infinity-Cache test uses the largest rank's shard; the chunk and
    // duplicate-pair tests below are per rank, so ranks may run different
    // matvec forms: that changes only the rounding of each rank's own
    // contribution, which is all-reduced before anything is decided, so the
    // ranks' decisions stay identical)
    const bool big = 144.0 * (double)ctx->max_no > 256.0 * 1024 * 1024;
    const bool use_t = force >= 0 ? force != 0 : W.npchunks > 0 || (big && !W.w32);
    if (use_t && !ctx->tobs_buf) ctx->tobs_buf = ctx->dalloc<double>(6 * (size_t)std::max(ctx->no, 1));
    if (!use_t && ctx->tobs_buf) { ctx->dfree(ctx->tobs_buf); ctx->tobs_buf = nullptr; }   // 48 B/obs back
    W.tobs = use_t ? ctx->tobs_buf : nullptr;
  }
  PcgOpts po{o.eta, o.min_linear_solver_iterations, std::max(1, o.max_linear_solver_iterations),
             o.preconditioner_type == BA_SCHUR_JACOBI ? 1 : 0};
  launch_point_elim(P, W, radius, s, ctx->take_norms());
  launch_cam_schur_diag(P, W, s, W.Sd);
  if (po.schur_jacobi && ctx->pcg_ndup > 0) launch_pcg_dup(P, W, s);   // (this rank's duplicate pairs)
  // exchange path: one 6 nvc vector per matvec crosses the ranks (the
  // camera slices are folded first, in the order the single-rank update
  // folds them, so both paths round identically).  The point-elimination
  // failure count is folded and all-reduced with the step's scalars at its
  // end (step_enqueue): a failed elimination on any rank makes the all-reduced
  // products non-finite, so every rank's CG stops alike and the step is
  // rejected on every rank (one collective fewer per LM iteration)
  const size_t tcount = (size_t)6 * ctx->nvc;
  W.pcg_folded = ctx->coll();
  if (ctx->coll()) ctx->allreduce(W.Sd, 27 * (size_t)ctx->nvc);
  if (ctx->nvc == 0) {
    if (W.pacc && P.np > 0) HIP_OK(hipMemsetAsync(W.vacc, 0, sizeof(double) * 3 * (size_t)P.np, s));   // (y = 0)
    // k_pcg_setup_fin, which clears them otherwise, does not run: a spin or
    // pivot failure left by an earlier DENSE_SCHUR solve of this context must
    // not be read back as this step's
    HIP_OK(hipMemsetAsync(W.scal + SL_CHOL_SPIN, 0, sizeof(double), s));
    HIP_OK(hipMemsetAsync(W.scal + SL_CHOL_BAD, 0, sizeof(double), s));
    return 0;
  }
  launch_pcg_setup(P, W, radius, po, s);
  int it = 0, batch = 4;
  for (;;) {
    for (int k = 0; k < batch && it < po.max_iter; ++k) {
      ++it;
      launch_pcg_matvec(P, W, W.pp, s);
      if (ctx->coll()) { launch_pcg_tfold(P, W, s); ctx->allreduce(W.tpart, tcount); }
      if (it % 10 == 0) {   // ceres residual_reset_period: r = b - S x
        launch_pcg_update(P, W, 1, it, po, s);
        launch_pcg_matvec(P, W, W.y, s);
        if (W.pacc) launch_pcg_vacc(P, W, it, true, s);   // vpt(y) itself
        if (ctx->coll()) { launch_pcg_tfold(P, W, s); ctx->allreduce(W.tpart, tcount); }
        launch_pcg_update(P, W, 2, it, po, s);
      } else {
        launch_pcg_update(P, W, 0, it, po, s);
        if (W.pacc) launch_pcg_vacc(P, W, it, false, s);
      }
    }
    ctx->read_scalars();
    if (ctx->h_scal[kNumSlots + PS_DONE] != 0.0 || it >= po.max_iter) break;
    batch = std::min(2 * batch, 32);
  }
  return (int)ctx->h_scal[kNumSlots + PS_ITER];
}

// Trust-region step phase: enqueue (the PCG reads its state record between
// batches of CG iterations) / read back.  Returns the linear-solver iterations.
// the per-observation Schur blocks of a step: fp32 or fp64, compact records,
// camera-major copies
// plain_w: the plain 18-value fp64 records whatever the options and the
// environment would select (ba_covariance_iterative reads them in its own
// passes; every later step decides again)
void step_w_storage(ba_ctx* ctx, const ba_options& o, bool plain_w = false) {
  DevWork& W = ctx->W;
  W.w32 = !plain_w && o.precision == BA_MIXED_FP32;
  if (W.w32 && !W.Wf) W.Wf = ctx->dalloc<float>(18 * (size_t)ctx->no);
  if (!W.w32 && !W.W) W.W = ctx->dalloc<double>(18 * (size_t)ctx->no);
  if (plain_w) {
    W.wcompact = W.pcgc = W.pcgjf = W.pacc = false;
    W.jdiag = W.jrfree;   // (the diagonal blocks J-free, as every ITERATIVE_SCHUR step forms them)
    if (W.jdiag && !W.prec) W.prec = ctx->dalloc<double>(16 * (size_t)std::max(ctx->np, 1));
    W.mcc_cam = ctx->rank == 0;
    return;
  }
  {
    // compact W records (ba_kernels.hip k_obs_w_rc<double, true>): the
    // J-free fp64 DENSE_SCHUR iteration with the fused point step (the only
    // W readers are then k_cam_schur_diag_c and k_schur_pairs_c);
    // BA_WCOMPACT=0 (diagnostics, read per solve) keeps the 18-double blocks
    const char* e = getenv("BA_WCOMPACT");
    W.wcompact = W.jrfree && ctx->nvc <= bahip::kWcCamsHost && !W.w32 && o.linear_solver == BA_DENSE_SCHUR &&
                 !(e && e[0] == '0');
  }
  {
    // the diagonal Schur blocks J-free (k_cam_schur_diag_rc) where they would
    // gather the 18-value W (ITERATIVE_SCHUR, or DENSE_SCHUR without compact
    // records): C4 3.53 vs 3.74 ms with the W-reading pass
    // (profiles/r04_v4_jdiag_tscat_ab.txt)
    W.jdiag = W.jrfree && !W.wcompact;
    if (W.jdiag && !W.prec) W.prec = ctx->dalloc<double>(16 * (size_t)std::max(ctx->np, 1));
    // the PCG point pass over the 16-value rank-2 records (k_obs_w_rc<.., PC>:
    // 128 B per observation fp64, 64 B fp32): only where nothing else reads
    // W — the diagonal blocks J-free, the fused point step, the products t_o,
    // no duplicate (camera, point) pairs, every point in the point-aligned
    // chunks — and K without skew.  BA_PCG_PC=0
    // (read per solve) keeps the 18-value records
    W.pcgc = false;
    const char* pe = getenv("BA_PCG_PC");
    const char* te = getenv("BA_PCG_T");
    if (!(pe && pe[0] == '0') && o.linear_solver == BA_ITERATIVE_SCHUR && W.jdiag && ctx->k_plain &&
        obs_w_pc_ok(ctx->P, W) && !(te && te[0] == '0')) {
      ensure_pcg(ctx);
      W.pcgc = W.npchunks > 0 && ctx->pcg_ndup == 0;
    }
    // fp64 beyond the LDS camera table (compact camera records): the point
    // pass forms those records itself instead of reading them
    // (k_pcg_point_jf, no W): C4 fixed radius 2.82 vs 3.14 ms per LM
    // iteration, along the trajectory 3.66 vs 3.89, C4 shard 0.50 vs 0.56;
    // with fp32 W (64-B records) the stored records win (C5 shard 3.65 vs
    // 3.81 ms: profiles/r05_v5_pcg_jfree_ab.txt).  BA_PCG_JF=0 / 1 (read per
    // solve) forces it off / on
    // the back substitution from the CG's accumulated point products (no J in
    // k_point_step_rc: k_pcg_vacc, the block-form model cost change).  With
    // fp32 W (MIXED_FP32) the products carry the stored fp32 blocks into the
    // back substitution as they carry them into the CG (a relative 1e-7
    // perturbation of the point step; the costs stay within the oracle
    // comparisons' 1e-9).  BA_PCG_PACC=0 (read per solve) recomputes J per
    // observation, in fp64
    W.pacc = false;
    const char* ae = getenv("BA_PCG_PACC");
    if (o.linear_solver == BA_ITERATIVE_SCHUR && W.jrfree && !(ae && ae[0] == '0')) {
      ensure_pcg(ctx);
      W.pacc = W.npchunks > 0;
    }
    W.mcc_cam = ctx->rank == 0;
    const char* je = getenv("BA_PCG_JF");
    const bool jf_ok = W.pcgc && ctx->P.nc > bahip::kLinLdsCamsHost;
    W.pcgjf = jf_ok && (je ? je[0] != '0' : !W.w32);
  }
}
int step_enqueue(ba_ctx* ctx, double radius, const ba_options& o) {
  const hipStream_t s = ctx->stream;
  DevProblem& P = ctx->P;
  DevWork& W = ctx->W;
  step_w_storage(ctx, o);
  // (SL_CHOL_BAD is cleared by k_cam_add_diag / k_pcg_setup_fin, the first
  // kernels that may set it, so no separate memset per step)
  int ls_iters = 1;
  if (o.linear_solver == BA_ITERATIVE_SCHUR) ls_iters = reduced_solve_pcg(ctx, radius, o);
  else reduced_solve_dense(ctx, radius);
  launch_cam_candidate(P, W, s);
  launch_backsub_candidate(P, W, s);
  // (DENSE_SCHUR under collectives: the elimination failures already
  // crossed the ranks with the packed S)
  const bool pcg = o.linear_solver == BA_ITERATIVE_SCHUR;
  const uint32_t step_sum = bit(SL_MCC_NEG) | bit(SL_CCOST) | bit(SL_STEP2_P) | bit(SL_CAND_BAD) | bit(SL_STEP_BAD) |
                            bit(SL_STEP2_C) | (ctx->coll() && !pcg ? 0u : bit(SL_ELIM_BAD));
  if (!ctx->coll()) {
    // folded by the scalar record's publish that follows every step
    // (ba_ctx::publish_scalars: one launch for the fold and the record)
    ctx->pend_sum |= step_sum;
    return ls_iters;
  }
  launch_reduce(W, step_sum | ctx->pend_sum, ctx->pend_max, s);
  ctx->pend_sum = ctx->pend_max = 0;
  if (ctx->coll()) {
    // MCC_NEG, CCOST, STEP2_P, CAND_BAD, STEP_BAD, CHOL_SPIN (+ ELIM_BAD: ITERATIVE_SCHUR)
    ctx->allreduce(W.scal + SL_MCC_NEG, pcg ? 7 : 6);
  }
  return ls_iters;
}

// after ctx->read_scalars()
StepResult step_result(ba_ctx* ctx, int ls_iters) {
  const double* h = ctx->h_scal;
  StepResult r;
  r.linear_ok = h[SL_ELIM_BAD] == 0.0 && h[SL_CHOL_BAD] == 0.0 && h[SL_STEP_BAD] == 0.0;
  r.mcc = -h[SL_MCC_NEG];
  r.cand_cost = h[SL_CAND_BAD] > 0.0 || !std::isfinite(h[SL_CCOST]) ? std::numeric_limits<double>::max() : h[SL_CCOST];
  r.step_norm = std::sqrt(h[SL_STEP2_P] + h[SL_STEP2_C]);
  r.ls_iters = ls_iters;
  r.spin = h[SL_CHOL_SPIN] != 0.0;
  return r;
}

void accept_candidate(ba_ctx* ctx) {
  std::swap(ctx->W.cams, ctx->W.cams_c);
  std::swap(ctx->W.pts, ctx->W.pts_c);
}

// Speculative linearisation at the last step's candidate, enqueued behind
// the step's scalar record: it runs while the host reads the record and
// decides, and it is the next iteration's linearisation when the step is
// accepted (the common case).  A rejected step re-linearises at x
// (ctx->lin_at_cand); the values are the same either way.  With collectives
// too: every rank enqueues the same linearisation (identical decisions), so
// the all-reduces keep one order across the ranks.  BA_SPEC_LIN=0: off
// (ba_ctx::read_env).
void spec_lin_enqueue(ba_ctx* ctx, const ba_options& o) {
  if (!ctx->spec_lin) return;
  // the kernels read W.cams / W.pts: point them at the candidate for the
  // enqueue only (restored on every exit, a throw included)
  struct Swap {
    ba_ctx* c;
    explicit Swap(ba_ctx* x) : c(x) { accept_candidate(c); }
    ~Swap() { accept_candidate(c); }
  } swap(ctx);
  linearize_enqueue(ctx, false, o.min_lm_diagonal, o.max_lm_diagonal, false, true);
  ctx->lin_at_cand = true;
}

void check_options(const ba_options& o) {
  if (o.linear_solver != BA_DENSE_SCHUR && o.linear_solver != BA_ITERATIVE_SCHUR)
    throw BaError{BA_ERR_INVALID_ARGUMENT, "unknown linear_solver " + std::to_string(o.linear_solver)};
  if (o.linear_solver == BA_ITERATIVE_SCHUR &&
      ((o.preconditioner_type != BA_JACOBI && o.preconditioner_type != BA_SCHUR_JACOBI) ||
       o.max_linear_solver_iterations < 1 || o.min_linear_solver_iterations < 0 || !(o.eta > 0.0)))
    throw BaError{BA_ERR_INVALID_ARGUMENT, "invalid ITERATIVE_SCHUR options"};
  if (o.precision != BA_FP64 && o.precision != BA_MIXED_FP32)
    throw BaError{BA_ERR_INVALID_ARGUMENT, "unknown precision " + std::to_string(o.precision)};
  if (o.precision == BA_MIXED_FP32 && o.linear_solver != BA_ITERATIVE_SCHUR)
    throw BaError{BA_ERR_INVALID_ARGUMENT, "BA_MIXED_FP32 requires BA_ITERATIVE_SCHUR"};
}

// ---------------------------------------------------------------------------
// ceres TrustRegionMinimizer (LM, monotonic) restated over the device phases
// ---------------------------------------------------------------------------
void solve(ba_ctx* ctx, const ba_options* opt, ba_summary* sum) {
  if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, "ba_solve before ba_set_problem"};
  ba_options o = options_or_default(opt);
  check_options(o);
  ctx->read_env();
  const double t0 = now_s();
  ctx->log.clear();
  ctx->t_lin = ctx->t_solve = 0.0;
  ba_summary S{};
  auto push = [&](const ba_iteration& it) { ctx->log.push_back(it); };
  double radius = o.initial_trust_region_radius, decrease_factor = 2.0;
  int consecutive_invalid = 0;

  double tl = now_s();
  LinResult L = linearize(ctx, o.jacobi_scaling != 0, o.min_lm_diagonal, o.max_lm_diagonal);
  ctx->t_lin += now_s() - tl;
  if (!o.jacobi_scaling) {
    // scale = 1: write ones (kernels always read scale arrays)
    std::vector<double> ones(3 * (size_t)ctx->np, 1.0), onesc(6 * (size_t)ctx->nvc, 1.0);
    HIP_OK(hipMemcpy(ctx->W.scale_p, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(ctx->W.scale_c, onesc.data(), onesc.size() * sizeof(double), hipMemcpyHostToDevice));
    L = linearize(ctx, false, o.min_lm_diagonal, o.max_lm_diagonal);
  }
  S.initial_cost = L.cost;
  if (!L.ok) {
    S.final_cost = L.cost;
    S.termination_type = BA_FAILURE;
    S.total_time_s = now_s() - t0;
    if (sum) *sum = S;
    return;
  }
  {
    ba_iteration it{};
    it.iteration = 0; it.step_is_valid = 1; it.step_is_successful = 1;
    it.cost = L.cost; it.gradient_max_norm = L.gmax; it.gradient_norm = L.gnorm;
    it.trust_region_radius = radius;
    it.iteration_time_s = now_s() - t0;
    push(it);
  }
  double x_cost = L.cost, x_norm = L.xnorm, gmax = L.gmax, gnorm = L.gnorm;
  int iteration = 0;
  int termination = BA_NO_CONVERGENCE;
  bool last_success = true;
  auto can_continue = [&]() {
    if (iteration >= o.max_num_iterations) { termination = BA_NO_CONVERGENCE; return false; }
    if (last_success && gmax <= o.gradient_tolerance) { termination = BA_CONVERGENCE; return false; }
    if (radius <= o.min_trust_region_radius) { termination = BA_CONVERGENCE; return false; }
    return true;
  };
  // a step enqueued right behind the last accepted step's linearisation
  // (its record arrived with the linearisation's): used if the solve goes on
  bool have_step = false;
  ctx->clear_pending();   // (an earlier solve may have thrown between the two enqueues)
  int spec_ls = 0;
  while (can_continue()) {
    const double ti = now_s();
    ++iteration;
    ba_iteration it{};
    it.iteration = iteration;
    double ts = now_s();
    int ls = spec_ls;
    if (!have_step) {
      // (after a rejected or invalid step the speculative linearisation at
      // its candidate replaced the one at x)
      if (ctx->lin_at_cand) linearize_enqueue(ctx, false, o.min_lm_diagonal, o.max_lm_diagonal, false, true);
      ls = step_enqueue(ctx, radius, o);
      ctx->publish_scalars();
      spec_lin_enqueue(ctx, o);
      ctx->wait_scalars();
    }
    have_step = false;
    StepResult st = step_result(ctx, ls);
    if (st.spin) {
      // a hand-off of the persistent factorisation never came (its grid
      // could not be fully resident, e.g. beside another process's kernels):
      // not a pivot failure.  Redo the step with the per-step launches (and
      // keep them for this context).  A spin of the per-step form's back
      // substitution (k_back_flow) has no fallback: BA_ERR_DEVICE.  Under
      // collectives the spin slot is all-reduced with the step's scalars, so
      // every rank redoes (or throws) together.
      if (!ctx->W.chol_persist && !ctx->W.chol_fuse && !ctx->W.chol_flow)
        throw BaError{BA_ERR_DEVICE, "dense Cholesky: a hand-off spin bound was hit"};
      ctx->W.chol_persist = false;
      ctx->W.chol_flow = false;   // (the split form's one-launch dataflow: per-step launches instead,
      ctx->W.chol_fuse = false;   //  and their in-launch panels: k_chol_panel launches)
      if (ctx->lin_at_cand) linearize_enqueue(ctx, false, o.min_lm_diagonal, o.max_lm_diagonal, false, true);
      ls = step_enqueue(ctx, radius, o);
      ctx->read_scalars();
      st = step_result(ctx, ls);
      if (st.spin) throw BaError{BA_ERR_DEVICE, "dense Cholesky: a hand-off spin bound was hit"};
    }
    ctx->t_solve += now_s() - ts;
    it.linear_solver_iterations = st.ls_iters;
    const bool valid = st.linear_ok && st.mcc > 0.0;
    it.model_cost_change = st.mcc;
    if (!valid) {
      if (++consecutive_invalid >= o.max_num_consecutive_invalid_steps) { termination = BA_FAILURE; break; }
      radius = radius / decrease_factor;
      decrease_factor *= 2.0;
      it.cost = x_cost; it.gradient_max_norm = gmax; it.gradient_norm = gnorm;
      it.trust_region_radius = radius; it.step_is_valid = 0; it.step_is_successful = 0;
      last_success = false;
      S.num_unsuccessful_steps++;
      it.iteration_time_s = now_s() - ti;
      push(it);
      continue;
    }
    consecutive_invalid = 0;
    it.step_norm = st.step_norm;
    if (st.step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) { termination = BA_CONVERGENCE; break; }
    const double cost_change = x_cost - st.cand_cost;
    it.cost_change = cost_change;
    if (std::fabs(cost_change) <= o.function_tolerance * x_cost) { termination = BA_CONVERGENCE; break; }
    const double rel = st.cand_cost >= std::numeric_limits<double>::max() ? std::numeric_limits<double>::lowest()
                                                                          : (x_cost - st.cand_cost) / st.mcc;
    it.relative_decrease = rel;
    if (rel > o.min_relative_decrease) {
      accept_candidate(ctx);
      radius = std::min(o.max_trust_region_radius, radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rel - 1.0, 3)));
      decrease_factor = 2.0;
      tl = now_s();
      // speculate: the next step at the new radius, unless the loop ends on
      // grounds already known (iteration cap, radius floor)
      const bool spec = iteration < o.max_num_iterations && radius > o.min_trust_region_radius;
      // the linearisation at the new x: already enqueued behind the step
      // (spec_lin_enqueue; its scalars are pending), else now
      if (!ctx->lin_at_cand) linearize_enqueue(ctx, false, o.min_lm_diagonal, o.max_lm_diagonal, false, spec);
      ctx->lin_at_cand = false;
      if (spec) {
        spec_ls = step_enqueue(ctx, radius, o);
      } else if (ctx->pend_sum | ctx->pend_max) {
        ctx->flush_norms();
        launch_reduce(ctx->W, ctx->pend_sum, ctx->pend_max, ctx->stream);
        ctx->pend_sum = ctx->pend_max = 0;
      }
      ctx->publish_scalars();
      if (spec) spec_lin_enqueue(ctx, o);
      ctx->wait_scalars();
      L = lin_result(ctx);
      have_step = spec;
      ctx->t_lin += now_s() - tl;
      if (!L.ok) { termination = BA_FAILURE; x_cost = L.cost; break; }
      x_cost = L.cost; x_norm = L.xnorm; gmax = L.gmax; gnorm = L.gnorm;
      last_success = true;
      S.num_successful_steps++;
      it.cost = x_cost; it.step_is_successful = 1;
    } else {
      radius = radius / decrease_factor;
      decrease_factor *= 2.0;
      last_success = false;
      S.num_unsuccessful_steps++;
      it.cost = st.cand_cost; it.step_is_successful = 0;
    }
    it.gradient_max_norm = gmax; it.gradient_norm = gnorm; it.trust_region_radius = radius; it.step_is_valid = 1;
    it.iteration_time_s = now_s() - ti;
    push(it);
  }
  S.final_cost = x_cost;
  S.termination_type = termination;
  S.num_iterations = iteration;
  S.total_time_s = now_s() - t0;
  S.linearize_time_s = ctx->t_lin;
  S.solve_time_s = ctx->t_solve;
  if (sum) *sum = S;
}

void get_params(ba_ctx* ctx, double* cams, double* pts) {
  if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, "no problem"};
  if (cams && ctx->nc) HIP_OK(hipMemcpy(cams, ctx->W.cams, 6 * sizeof(double) * ctx->nc, hipMemcpyDeviceToHost));
  if (pts && ctx->np) HIP_OK(hipMemcpy(pts, ctx->W.pts, 3 * sizeof(double) * ctx->np, hipMemcpyDeviceToHost));
}

// compact index of a requested camera (-1: constant) and the check of a
// requested point, shared by the covariance entry points (fn: the entry
// point's name for messages)
int cov_cam_index(const ba_ctx* ctx, const std::string& fn, int c) {
  if (c < 0 || c >= ctx->nc)
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": camera index " + std::to_string(c) + " out of range"};
  const int v = ctx->h_vc[c];
  if (v < 0 && !ctx->cam_fixed_h[c])
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": camera " + std::to_string(c) +
                                               " is variable but has no observation"};
  return v;
}
void cov_check_point(const ba_ctx* ctx, const std::string& fn, int p) {
  if (p < 0 || p >= ctx->np)
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": point index " + std::to_string(p) + " out of range"};
  if (!ctx->h_pt_var[p] && !ctx->pt_fixed_h[p])
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": point " + std::to_string(p) +
                                               " is variable but has no observation"};
}

// ---------------------------------------------------------------------------
// ceres::Covariance (defaults) for any pair of parameter blocks, and the
// leverages J_o Sigma J_o^T of observations (ba_covariance, ba_covariance_ex;
// fn: the entry point's name for messages): the undamped reduced system
// through a DENSE_SCHUR step's own passes and factorisation, then ba_cov.hip
// ---------------------------------------------------------------------------
void covariance(ba_ctx* ctx, const ba_covariance_request_ex* rx, const std::string& fn) {
  if (!rx) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": request is NULL"};
  const ba_covariance_request* req = &rx->base;
  if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, fn + " before ba_set_problem"};
  if (ctx->has_comm())
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": not available on a context with a communicator"};
  const int m = req->n_cam_pairs, k = req->n_points;
  const int ncp = rx->n_cam_pt, npp = rx->n_pt_pairs, nlev = rx->n_lev;
  if (m < 0 || k < 0 || (m > 0 && (!req->cam_pairs || !req->cam_cov)) || (k > 0 && (!req->points || !req->pt_cov)) ||
      ncp < 0 || npp < 0 || nlev < 0 || (ncp > 0 && (!rx->cam_pt || !rx->cam_pt_cov)) ||
      (npp > 0 && (!rx->pt_pairs || !rx->pt_pt_cov)) || (nlev > 0 && !rx->leverage) ||
      (nlev > 0 && !rx->lev_obs && nlev != ctx->no))
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": bad sizes or missing array"};
  auto cam_index = [&](int c) { return cov_cam_index(ctx, fn, c); };
  auto check_point = [&](int p) { cov_check_point(ctx, fn, p); };
  std::vector<int2> pairs_h(m), cp_h(ncp);
  for (int q = 0; q < m; ++q) {
    const int v0 = cam_index(req->cam_pairs[2 * q]), v1 = cam_index(req->cam_pairs[2 * q + 1]);
    pairs_h[q] = make_int2(v0, v1);
  }
  for (int q = 0; q < k; ++q) check_point(req->points[q]);
  for (int q = 0; q < ncp; ++q) {
    const int v = cam_index(rx->cam_pt[2 * q]);
    check_point(rx->cam_pt[2 * q + 1]);
    cp_h[q] = make_int2(v, rx->cam_pt[2 * q + 1]);
  }
  for (int q = 0; q < 2 * npp; ++q) check_point(rx->pt_pairs[q]);
  // leverages: the points that have a requested observation (increasing,
  // each once), the running count of their observations (a point's slots in
  // the result scratch) and the scratch slot of each requested observation
  std::vector<int> lev_idx(nlev), lev_pts, lev_off;
  size_t lev_slots = 0;
  if (nlev > 0) {
    const int no = ctx->no;
    const std::vector<int>& off = ctx->h_pt_off;
    if (!rx->lev_obs) {   // every observation: the inverse of perm, every observed point
      for (int s = 0; s < no; ++s) lev_idx[ctx->perm[s]] = s;
      for (int p = 0; p < ctx->np; ++p)
        if (off[p + 1] > off[p]) { lev_pts.push_back(p); lev_off.push_back(off[p]); }
      lev_slots = (size_t)no;
    } else {
      std::vector<int> inv(no), pt_of(nlev), slot0(ctx->np, -1);
      for (int s = 0; s < no; ++s) inv[ctx->perm[s]] = s;
      for (int q = 0; q < nlev; ++q) {
        const int o = rx->lev_obs[q];
        if (o < 0 || o >= no)
          throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": observation index " + std::to_string(o) + " out of range"};
        pt_of[q] = (int)(std::upper_bound(off.begin(), off.end(), inv[o]) - off.begin()) - 1;
        slot0[pt_of[q]] = 0;
      }
      for (int p = 0; p < ctx->np; ++p)
        if (slot0[p] == 0) {
          slot0[p] = (int)lev_slots;
          lev_pts.push_back(p);
          lev_off.push_back((int)lev_slots);
          lev_slots += (size_t)(off[p + 1] - off[p]);
        }
      for (int q = 0; q < nlev; ++q) lev_idx[q] = slot0[pt_of[q]] + inv[rx->lev_obs[q]] - off[pt_of[q]];
    }
  }
  HIP_OK(hipSetDevice(ctx->device));
  ba_options o = options_or_default(nullptr);   // DENSE_SCHUR, fp64
  ctx->read_env();
  const hipStream_t s = ctx->stream;
  struct Events {
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } ev;
  for (hipEvent_t& x : ev.e) HIP_OK(hipEventCreate(&x));
  HIP_OK(hipEventRecord(ev.e[0], s));
  const LinResult L = linearize(ctx, true, o.min_lm_diagonal, o.max_lm_diagonal);
  if (!L.ok) throw BaError{BA_ERR_SINGULAR, fn + ": the linearisation is not finite"};
  DevWork& W = ctx->W;
  if (nlev > 0 && W.jrfree) {
    // the iteration never stores J: write the records for the leverage pass,
    // as ba_linearize does for its read-back (its cost partials are not this
    // call's: fold and clear them so no later reduction counts them)
    if (!W.JR) W.JR = ctx->dalloc<double>((size_t)(bahip::jr_ja_host(ctx->P.nc) + 8) * ctx->no);
    bahip::launch_linearize_jr(ctx->P, W, s);
    launch_reduce(W, bit(SL_COST) | bit(SL_LIN_BAD), 0, s);
  }
  step_w_storage(ctx, o);
  // an infinite radius: every D = sqrt(diag / radius) of the LM diagonal is
  // exactly zero, so the step's passes form the undamped system
  const double radius = std::numeric_limits<double>::infinity();
  for (int attempt = 0;; ++attempt) {
    form_reduced_dense(ctx, radius, false);   // (ensure_dense refuses a system too large for DENSE_SCHUR)
    HIP_OK(hipEventRecord(ev.e[1], s));
    launch_cholesky_solve2(ctx->P, W, ++ctx->chol_epoch, s);
    HIP_OK(hipEventRecord(ev.e[2], s));
    launch_reduce(W, bit(SL_ELIM_BAD), 0, s);
    ctx->read_scalars();
    const double* h = ctx->h_scal;
    if (ctx->n > 0 && h[SL_CHOL_SPIN] != 0.0) {
      // a hand-off of the factorisation never came: as in solve(), once more
      // with the per-step launches (kept for this context)
      if (attempt > 0 || (!W.chol_persist && !W.chol_fuse && !W.chol_flow))
        throw BaError{BA_ERR_DEVICE, "dense Cholesky: a hand-off spin bound was hit"};
      W.chol_persist = W.chol_flow = W.chol_fuse = false;
      continue;
    }
    if (h[SL_ELIM_BAD] != 0.0)
      throw BaError{BA_ERR_SINGULAR, fn + ": " + std::to_string((long long)h[SL_ELIM_BAD]) +
                                         " point block(s) not positive definite"};
    if (ctx->n > 0 && h[SL_CHOL_BAD] != 0.0)
      throw BaError{BA_ERR_SINGULAR, fn + ": the reduced camera system is not positive definite"};
    break;
  }
  // request and result staging (freed on every exit)
  enum { D_PAIRS, D_CAM, D_PTS, D_PT, D_CP, D_CPOUT, D_PQ, D_PQOUT, D_LPTS, D_LOFF, D_LIDX, D_HBUF, D_LEV, D_N };
  struct Dev {
    void* p[D_N] = {};
    ~Dev() { for (void* x : p) if (x) (void)hipFree(x); }
  } d;
  auto stage = [&](int slot, const void* src, size_t bytes) {
    HIP_OK(hipMalloc(&d.p[slot], bytes));
    if (src) HIP_OK(hipMemcpyAsync(d.p[slot], src, bytes, hipMemcpyHostToDevice, s));
  };
  if (m > 0) {
    stage(D_PAIRS, pairs_h.data(), sizeof(int2) * (size_t)m);
    stage(D_CAM, nullptr, sizeof(double) * 36 * (size_t)m);
  }
  if (k > 0) {
    stage(D_PTS, req->points, sizeof(int) * (size_t)k);
    stage(D_PT, nullptr, sizeof(double) * 9 * (size_t)k);
  }
  if (ncp > 0) {
    stage(D_CP, cp_h.data(), sizeof(int2) * (size_t)ncp);
    stage(D_CPOUT, nullptr, sizeof(double) * 18 * (size_t)ncp);
  }
  if (npp > 0) {
    stage(D_PQ, rx->pt_pairs, sizeof(int2) * (size_t)npp);
    stage(D_PQOUT, nullptr, sizeof(double) * 9 * (size_t)npp);
  }
  if (nlev > 0) {
    stage(D_LPTS, lev_pts.data(), sizeof(int) * lev_pts.size());
    stage(D_LOFF, lev_off.data(), sizeof(int) * lev_off.size());
    stage(D_LIDX, lev_idx.data(), sizeof(int) * (size_t)nlev);
    stage(D_HBUF, nullptr, sizeof(double) * 4 * lev_slots);
    stage(D_LEV, nullptr, sizeof(double) * 4 * (size_t)nlev);
  }
  launch_cov_inverse(ctx->P, W, s);
  HIP_OK(hipEventRecord(ev.e[3], s));
  launch_cov_cam_blocks(ctx->P, W, static_cast<const int2*>(d.p[D_PAIRS]), m, static_cast<double*>(d.p[D_CAM]), s);
  launch_cov_points(ctx->P, W, static_cast<const int*>(d.p[D_PTS]), k, static_cast<double*>(d.p[D_PT]), s);
  launch_cov_cam_pt(ctx->P, W, static_cast<const int2*>(d.p[D_CP]), ncp, static_cast<double*>(d.p[D_CPOUT]), s);
  launch_cov_pt_pairs(ctx->P, W, static_cast<const int2*>(d.p[D_PQ]), npp, static_cast<double*>(d.p[D_PQOUT]), s);
  launch_cov_leverage(ctx->P, W, static_cast<const int*>(d.p[D_LPTS]), static_cast<const int*>(d.p[D_LOFF]),
                      (int)lev_pts.size(), static_cast<double*>(d.p[D_HBUF]), static_cast<const int*>(d.p[D_LIDX]), nlev,
                      static_cast<double*>(d.p[D_LEV]), s);
  HIP_OK(hipGetLastError());
  auto fetch = [&](double* dst, int slot, size_t count) {
    if (count > 0) HIP_OK(hipMemcpyAsync(dst, d.p[slot], sizeof(double) * count, hipMemcpyDeviceToHost, s));
  };
  fetch(req->cam_cov, D_CAM, 36 * (size_t)m);
  fetch(req->pt_cov, D_PT, 9 * (size_t)k);
  fetch(rx->cam_pt_cov, D_CPOUT, 18 * (size_t)ncp);
  fetch(rx->pt_pt_cov, D_PQOUT, 9 * (size_t)npp);
  fetch(rx->leverage, D_LEV, 4 * (size_t)nlev);
  // W.S held L^-T: back to zeros, its state before the first step (the
  // steps rewrite its lower triangle only)
  if (ctx->n > 0) HIP_OK(hipMemsetAsync(W.S, 0, sizeof(double) * (size_t)(ctx->n + 1) * std::max(ctx->ld, 1), s));
  HIP_OK(hipEventRecord(ev.e[4], s));
  HIP_OK(hipStreamSynchronize(s));
  for (size_t i = 0; i < 36 * (size_t)m; ++i)
    if (!std::isfinite(req->cam_cov[i]))
      throw BaError{BA_ERR_SINGULAR, fn + ": camera block " + std::to_string(i / 36) + " is not finite"};
  for (size_t i = 0; i < 9 * (size_t)k; ++i)
    if (!std::isfinite(req->pt_cov[i]))
      throw BaError{BA_ERR_SINGULAR, fn + ": the block of point " + std::to_string(req->points[i / 9]) +
                                         " is not finite"};
  for (size_t i = 0; i < 18 * (size_t)ncp; ++i)
    if (!std::isfinite(rx->cam_pt_cov[i]))
      throw BaError{BA_ERR_SINGULAR, fn + ": camera-point block " + std::to_string(i / 18) + " is not finite"};
  for (size_t i = 0; i < 9 * (size_t)npp; ++i)
    if (!std::isfinite(rx->pt_pt_cov[i]))
      throw BaError{BA_ERR_SINGULAR, fn + ": point-point block " + std::to_string(i / 9) + " is not finite"};
  for (size_t i = 0; i < 4 * (size_t)nlev; ++i)
    if (!std::isfinite(rx->leverage[i]))
      throw BaError{BA_ERR_SINGULAR, fn + ": leverage " + std::to_string(i / 4) + " is not finite"};
  ctx->cov_ms.assign(4, 0.0);
  for (int i = 0; i < 4; ++i) {
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, ev.e[i], ev.e[i + 1]));
    ctx->cov_ms[i] = ms;
  }
}

// ---------------------------------------------------------------------------
// ba_covariance_iterative: ba_covariance's request from block columns of
// S_scaled^-1 solved by multi-column PCG on the implicit reduced camera system
// (ba_cov_pcg.hip).  Prologue as covariance(): linearisation with its Jacobi
// scaling, the step's W records (the plain fp64 form), an infinite radius.
// ---------------------------------------------------------------------------
void mcg_ensure(ba_ctx* ctx, int B) {
  const int R = 6 * B;
  if (ctx->mcg_cols >= R) return;
  bahip::McgBufs& b = ctx->mcg;
  for (double* p : {b.X, b.Rv, b.Z, b.Pv, b.Q, b.T, b.Vp, b.part}) ctx->dfree(p);
  b.X = b.Rv = b.Z = b.Pv = b.Q = b.T = b.Vp = b.part = nullptr;
  ctx->mcg_cols = 0;
  const size_t vec = (size_t)std::max(ctx->nvc, 1) * 6 * R;
  const size_t groups = (size_t)(std::max(ctx->nvc, 1) + bahip::kMcgGroup - 1) / bahip::kMcgGroup;
  b.X = ctx->dalloc<double>(vec);
  b.Rv = ctx->dalloc<double>(vec);
  b.Z = ctx->dalloc<double>(vec);
  b.Pv = ctx->dalloc<double>(vec);
  b.Q = ctx->dalloc<double>(vec);
  b.T = ctx->dalloc<double>(vec * (size_t)std::max(ctx->W.pcg_G, 1));
  b.Vp = ctx->dalloc<double>((size_t)std::max(ctx->np, 1) * 3 * R);   // (the large one: why B is small)
  b.part = ctx->dalloc<double>(3 * groups * R);
  if (!b.st) b.st = ctx->dalloc<double>(bahip::kMcgState);
  ctx->mcg_cols = R;
}

void covariance_iterative(ba_ctx* ctx, const ba_covariance_request* req, const ba_cov_iter_options* opt_in,
                          ba_cov_iter_info* info) {
  const std::string fn = "ba_covariance_iterative";
  if (!req) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": request is NULL"};
  if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, fn + " before ba_set_problem"};
  if (ctx->has_comm())
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": not available on a context with a communicator"};
  ba_cov_iter_options co;
  ba_covariance_iterative_defaults(&co);
  if (opt_in) co = *opt_in;
  if (!(co.tolerance > 0.0) || !std::isfinite(co.tolerance))
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": tolerance must be positive and finite"};
  if (co.max_iterations < 1) throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": max_iterations < 1"};
  if (co.preconditioner_type != BA_JACOBI && co.preconditioner_type != BA_SCHUR_JACOBI)
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": unknown preconditioner"};
  const int m = req->n_cam_pairs, k = req->n_points;
  if (m < 0 || k < 0 || (m > 0 && (!req->cam_pairs || !req->cam_cov)) || (k > 0 && (!req->points || !req->pt_cov)))
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": bad sizes or missing array"};
  std::vector<int2> pairs_h(m);
  for (int q = 0; q < m; ++q) {
    const int v0 = cov_cam_index(ctx, fn, req->cam_pairs[2 * q]), v1 = cov_cam_index(ctx, fn, req->cam_pairs[2 * q + 1]);
    pairs_h[q] = make_int2(v0, v1);
  }
  for (int q = 0; q < k; ++q) cov_check_point(ctx, fn, req->points[q]);
  // column cameras, increasing: column j of a pair with both cameras
  // variable, every variable observer of a requested variable point
  std::vector<char> is_col(std::max(ctx->nvc, 1), 0);
  for (const int2& pr : pairs_h)
    if (pr.x >= 0 && pr.y >= 0) is_col[pr.y] = 1;
  for (int q = 0; q < k; ++q) {
    const int p = req->points[q];
    if (!ctx->h_pt_var[p]) continue;
    for (int o = ctx->h_pt_off[p]; o < ctx->h_pt_off[p + 1]; ++o) {
      const int v = ctx->h_vc[ctx->h_obs_cam[o]];
      if (v >= 0) is_col[v] = 1;
    }
  }
  std::vector<int> cols;
  for (int v = 0; v < ctx->nvc; ++v)
    if (is_col[v]) cols.push_back(v);
  // the pair requests with a column, ordered by column camera; col_off[c]: the
  // first of column camera cols[c]
  std::vector<int> ord, col_off(cols.size() + 1, 0);
  {
    std::vector<int> rank(std::max(ctx->nvc, 1), -1);
    for (size_t c = 0; c < cols.size(); ++c) rank[cols[c]] = (int)c;
    for (int q = 0; q < m; ++q)
      if (pairs_h[q].x >= 0 && pairs_h[q].y >= 0) ++col_off[rank[pairs_h[q].y] + 1];
    for (size_t c = 0; c < cols.size(); ++c) col_off[c + 1] += col_off[c];
    ord.resize(col_off[cols.size()]);
    std::vector<int> fill(col_off.begin(), col_off.end() - 1);
    for (int q = 0; q < m; ++q)
      if (pairs_h[q].x >= 0 && pairs_h[q].y >= 0) ord[fill[rank[pairs_h[q].y]]++] = q;
  }
  // column cameras per pass: BA_COV_PCG_COLS (diagnostics, read per call) forces 1, 2 or 4
  int B = cols.size() >= 3 ? 4 : (cols.size() == 2 ? 2 : 1);
  if (const char* be = getenv("BA_COV_PCG_COLS")) {
    const int f = atoi(be);
    if (f == 1 || f == 2 || f == 4) B = f;
  }
  const int R = 6 * B;
  HIP_OK(hipSetDevice(ctx->device));
  ba_options o = options_or_default(nullptr);
  ctx->read_env();
  const hipStream_t s = ctx->stream;
  struct Events {
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } ev;
  for (hipEvent_t& x : ev.e) HIP_OK(hipEventCreate(&x));
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  auto add_ms = [&](int slot, hipEvent_t a, hipEvent_t b) {
    float t = 0.0f;
    HIP_OK(hipEventElapsedTime(&t, a, b));
    ms[slot] += t;
  };
  HIP_OK(hipEventRecord(ev.e[0], s));
  const LinResult L = linearize(ctx, true, o.min_lm_diagonal, o.max_lm_diagonal);
  if (!L.ok) throw BaError{BA_ERR_SINGULAR, fn + ": the linearisation is not finite"};
  DevProblem& P = ctx->P;
  DevWork& W = ctx->W;
  step_w_storage(ctx, o, true);
  ensure_pcg(ctx);
  const double radius = std::numeric_limits<double>::infinity();   // every D = sqrt(diag / radius) is exactly 0
  const bool sj = co.preconditioner_type == BA_SCHUR_JACOBI;
  launch_point_elim(P, W, radius, s, nullptr);
  launch_cam_schur_diag(P, W, s, W.Sd);
  if (sj && ctx->pcg_ndup > 0) launch_pcg_dup(P, W, s);
  launch_reduce(W, bit(SL_ELIM_BAD), 0, s);
  ctx->read_scalars();
  if (ctx->h_scal[SL_ELIM_BAD] != 0.0)
    throw BaError{BA_ERR_SINGULAR, fn + ": " + std::to_string((long long)ctx->h_scal[SL_ELIM_BAD]) +
                                       " point block(s) not positive definite"};
  mcg_ensure(ctx, B);
  const bahip::McgBufs& mb = ctx->mcg;
  std::vector<double> hst(bahip::kMcgState, 0.0);
  if (ctx->nvc > 0) {
    HIP_OK(hipMemsetAsync(mb.st, 0, sizeof(double) * bahip::kMcgState, s));
    bahip::launch_mcg_blocks(P, W, sj, mb.st, s);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(hst.data(), mb.st, sizeof(double) * bahip::kMcgState, hipMemcpyDeviceToHost, s));
  }
  HIP_OK(hipEventRecord(ev.e[1], s));
  HIP_OK(hipStreamSynchronize(s));
  add_ms(0, ev.e[0], ev.e[1]);
  if (hst[bahip::MS_BADBLK] != 0.0)
    throw BaError{BA_ERR_SINGULAR, fn + ": a preconditioner block is not positive definite"};
  // request and result staging (freed on every exit)
  enum { D_PAIRS, D_ORD, D_CAM, D_PTS, D_ACC, D_PT, D_N };
  struct Dev {
    void* p[D_N] = {};
    ~Dev() { for (void* x : p) if (x) (void)hipFree(x); }
  } d;
  auto stage = [&](int slot, const void* src, size_t bytes) {
    HIP_OK(hipMalloc(&d.p[slot], std::max<size_t>(bytes, 8)));
    if (src && bytes) HIP_OK(hipMemcpyAsync(d.p[slot], src, bytes, hipMemcpyHostToDevice, s));
    else if (bytes) HIP_OK(hipMemsetAsync(d.p[slot], 0, bytes, s));   // (zeros: the blocks of constant cameras)
  };
  if (m > 0) {
    stage(D_PAIRS, pairs_h.data(), sizeof(int2) * (size_t)m);
    stage(D_ORD, ord.data(), sizeof(int) * ord.size());
    stage(D_CAM, nullptr, sizeof(double) * 36 * (size_t)m);
  }
  if (k > 0) {
    stage(D_PTS, req->points, sizeof(int) * (size_t)k);
    stage(D_ACC, nullptr, sizeof(double) * 9 * (size_t)k);
    stage(D_PT, nullptr, sizeof(double) * 9 * (size_t)k);
  }
  int n_conv = 0, iters_used = 0;
  double max_res = 0.0;
  bool broke = false;
  const int ng = (std::max(ctx->nvc, 1) + bahip::kMcgGroup - 1) / bahip::kMcgGroup;
  std::vector<double> hpart((size_t)ng * R);
  for (size_t c0 = 0; c0 < cols.size(); c0 += (size_t)B) {
    const int nb = (int)std::min<size_t>((size_t)B, cols.size() - c0);
    bahip::McgPass ps;
    for (int b = 0; b < bahip::kMcgMaxB; ++b) ps.cc[b] = b < nb ? cols[c0 + b] : -1;
    HIP_OK(hipEventRecord(ev.e[1], s));
    bahip::launch_mcg_init(P, W, mb, B, ps, co.tolerance, s);
    // iterations in growing batches; the state record between them (the
    // kernels of a pass whose columns are all done return at once)
    int it = 0, batch = 4;
    for (;;) {
      for (int j = 0; j < batch && it < co.max_iterations; ++j) {
        ++it;
        bahip::launch_mcg_matvec(P, W, mb, B, mb.Pv, false, s);
        if (it % 10 == 0) {   // the residual reset of the single-vector CG: r = e - S x
          bahip::launch_mcg_update(P, W, mb, B, ps, 1, it, co.tolerance, co.max_iterations, s);
          bahip::launch_mcg_matvec(P, W, mb, B, mb.X, false, s);
          bahip::launch_mcg_update(P, W, mb, B, ps, 2, it, co.tolerance, co.max_iterations, s);
        } else {
          bahip::launch_mcg_update(P, W, mb, B, ps, 0, it, co.tolerance, co.max_iterations, s);
        }
      }
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(hst.data(), mb.st, sizeof(double) * bahip::kMcgState, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      if (hst[bahip::MS_ALLDONE] != 0.0 || it >= co.max_iterations) break;
      batch = std::min(2 * batch, 32);
    }
    HIP_OK(hipEventRecord(ev.e[2], s));
    // the true residual of the final X by one more matvec; its point pass
    // leaves V_p of every point for the point gathers
    bahip::launch_mcg_matvec(P, W, mb, B, mb.X, true, s);
    bahip::launch_mcg_update(P, W, mb, B, ps, 3, it, co.tolerance, co.max_iterations, s);
    HIP_OK(hipMemcpyAsync(hpart.data(), mb.part + 2 * (size_t)ng * R, sizeof(double) * (size_t)ng * R,
                          hipMemcpyDeviceToHost, s));
    bahip::launch_mcg_gather_cam(P, W, mb, B, ps, static_cast<const int2*>(d.p[D_PAIRS]),
                                 static_cast<const int*>(d.p[D_ORD]), col_off[c0], col_off[c0 + nb],
                                 static_cast<double*>(d.p[D_CAM]), s);
    bahip::launch_mcg_gather_pt(P, W, mb, B, ps, static_cast<const int*>(d.p[D_PTS]), k,
                                static_cast<double*>(d.p[D_ACC]), s);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(ev.e[3], s));
    HIP_OK(hipStreamSynchronize(s));
    add_ms(1, ev.e[1], ev.e[2]);
    add_ms(2, ev.e[2], ev.e[3]);
    for (int r = 0; r < 6 * nb; ++r) {
      if (hst[bahip::mcg_slot(bahip::MC_BAD, r)] != 0.0) broke = true;
      if (hst[bahip::mcg_slot(bahip::MC_CONV, r)] != 0.0) ++n_conv;
      iters_used = std::max(iters_used, (int)hst[bahip::mcg_slot(bahip::MC_ITERS, r)]);
      double rr = 0.0;
      for (int g = 0; g < ng; ++g) rr += hpart[(size_t)g * R + r];
      const double res = std::sqrt(rr);
      max_res = std::isfinite(res) ? std::max(max_res, res) : std::numeric_limits<double>::infinity();
    }
    if (broke) break;
  }
  if (broke)
    throw BaError{BA_ERR_SINGULAR, fn + ": the conjugate gradients broke down (the reduced camera system or its "
                                        "preconditioner is not positive definite)"};
  HIP_OK(hipEventRecord(ev.e[3], s));
  bahip::launch_mcg_pt_finish(P, W, static_cast<const int*>(d.p[D_PTS]), k, static_cast<const double*>(d.p[D_ACC]),
                              static_cast<double*>(d.p[D_PT]), s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(ev.e[2], s));
  if (m > 0) HIP_OK(hipMemcpyAsync(req->cam_cov, d.p[D_CAM], sizeof(double) * 36 * (size_t)m, hipMemcpyDeviceToHost, s));
  if (k > 0) HIP_OK(hipMemcpyAsync(req->pt_cov, d.p[D_PT], sizeof(double) * 9 * (size_t)k, hipMemcpyDeviceToHost, s));
  HIP_OK(hipEventRecord(ev.e[4], s));
  HIP_OK(hipStreamSynchronize(s));
  add_ms(2, ev.e[3], ev.e[2]);
  add_ms(3, ev.e[2], ev.e[4]);
  for (size_t i = 0; i < 36 * (size_t)m; ++i)
    if (!std::isfinite(req->cam_cov[i]))
      throw BaError{BA_ERR_SINGULAR, fn + ": camera block " + std::to_string(i / 36) + " is not finite"};
  for (size_t i = 0; i < 9 * (size_t)k; ++i)
    if (!std::isfinite(req->pt_cov[i]))
      throw BaError{BA_ERR_SINGULAR, fn + ": the block of point " + std::to_string(req->points[i / 9]) +
                                         " is not finite"};
  if (info) {
    info->n_columns = 6 * (int)cols.size();
    info->n_converged = n_conv;
    info->max_iterations_used = iters_used;
    info->reserved = 0;
    info->max_residual = max_res;
    for (int i = 0; i < 4; ++i) info->ms[i] = ms[i];
  }
}

// ba_covariance_iterative_bench: matvec timings on the iterative covariance's
// prologue state (cols = 0: launch_pcg_matvec on the same plain W records)
void covariance_iterative_bench(ba_ctx* ctx, int cols, int reps, int warmup, double* ms) {
  const std::string fn = "ba_covariance_iterative_bench";
  if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, fn + " before ba_set_problem"};
  if (ctx->has_comm())
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": not available on a context with a communicator"};
  if ((cols != 0 && cols != 1 && cols != 2 && cols != 4) || reps < 1 || warmup < 0 || !ms || ctx->nvc == 0)
    throw BaError{BA_ERR_INVALID_ARGUMENT, fn + ": bad arguments"};
  HIP_OK(hipSetDevice(ctx->device));
  ba_options o = options_or_default(nullptr);
  ctx->read_env();
  const hipStream_t s = ctx->stream;
  const LinResult L = linearize(ctx, true, o.min_lm_diagonal, o.max_lm_diagonal);
  if (!L.ok) throw BaError{BA_ERR_SINGULAR, fn + ": the linearisation is not finite"};
  DevProblem& P = ctx->P;
  DevWork& W = ctx->W;
  step_w_storage(ctx, o, true);
  ensure_pcg(ctx);
  launch_point_elim(P, W, std::numeric_limits<double>::infinity(), s, nullptr);
  launch_cam_schur_diag(P, W, s, W.Sd);
  launch_reduce(W, bit(SL_ELIM_BAD), 0, s);
  const int B = std::max(cols, 1);
  mcg_ensure(ctx, B);
  const bahip::McgBufs& mb = ctx->mcg;
  HIP_OK(hipMemsetAsync(mb.st, 0, sizeof(double) * bahip::kMcgState, s));
  bahip::launch_mcg_blocks(P, W, true, mb.st, s);
  bahip::McgPass ps;
  for (int b = 0; b < bahip::kMcgMaxB; ++b) ps.cc[b] = b < B ? std::min(b, ctx->nvc - 1) : -1;
  bahip::launch_mcg_init(P, W, mb, B, ps, 1e-300, s);   // (p = M e: a multi-vector to multiply)
  // the single-vector form reads its state record's PS_DONE: as a step's setup leaves it
  const bool had_tobs = W.tobs != nullptr;
  if (cols == 0) {
    W.tobs = nullptr;   // (the W-gathering camera pass: the same records as the multi-column form)
    HIP_OK(hipMemsetAsync(W.scal + kNumSlots, 0, sizeof(double) * kPcgState, s));
    HIP_OK(hipMemcpyAsync(W.pp, mb.Pv, sizeof(double) * (size_t)ctx->n, hipMemcpyDeviceToDevice, s));
  }
  std::vector<hipEvent_t> ev(2 * (size_t)reps, nullptr);
  struct Guard {
    std::vector<hipEvent_t>& e;
    ~Guard() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } guard{ev};
  for (hipEvent_t& x : ev) HIP_OK(hipEventCreate(&x));
  for (int i = 0; i < warmup + reps; ++i) {
    if (i >= warmup) HIP_OK(hipEventRecord(ev[2 * (size_t)(i - warmup)], s));
    if (cols == 0) launch_pcg_matvec(P, W, W.pp, s);
    else bahip::launch_mcg_matvec(P, W, mb, B, mb.Pv, true, s);
    if (i >= warmup) HIP_OK(hipEventRecord(ev[2 * (size_t)(i - warmup) + 1], s));
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s));
  if (cols == 0 && had_tobs) W.tobs = ctx->tobs_buf;
  for (int i = 0; i < reps; ++i) {
    float t = 0.0f;
    HIP_OK(hipEventElapsedTime(&t, ev[2 * (size_t)i], ev[2 * (size_t)i + 1]));
    ms[i] = t;
  }
}

// ---------------------------------------------------------------------------
// ba_debug_factor: the DENSE_SCHUR factorisation + back substitution of a
// step (launch_cholesky_solve2) on a caller-supplied system of the problem's
// order.  The overlapped form forms S inside its own launch and cannot take an
// injected matrix: it is not reachable from here (its bitwise test against the
// separate passes covers it).
// ---------------------------------------------------------------------------
void debug_factor(ba_ctx* ctx, const double* S_in, const double* rhs_in, double* L, double* V, double* y, int* ok) {
  if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, "ba_debug_factor before ba_set_problem"};
  if (ctx->has_comm())
    throw BaError{BA_ERR_INVALID_ARGUMENT, "ba_debug_factor: not available on a context with a communicator"};
  if (ctx->n == 0) throw BaError{BA_ERR_INVALID_ARGUMENT, "ba_debug_factor: the problem has no variable observed camera"};
  if (!S_in || !rhs_in) throw BaError{BA_ERR_INVALID_ARGUMENT, "ba_debug_factor: S_in / rhs_in is NULL"};
  HIP_OK(hipSetDevice(ctx->device));
  ensure_dense(ctx);   // (refuses a system too large for DENSE_SCHUR)
  const hipStream_t s = ctx->stream;
  DevWork& W = ctx->W;
  const size_t n = (size_t)ctx->n, ld = (size_t)ctx->ld, T = (n + 63) / 64;
  // the (n+1) x ld trapezoid: lower triangle of S_in, row n = rhs; what the
  // kernels do not read stays zero (the solver's state)
  std::vector<double> m((n + 1) * ld, 0.0);
  for (size_t i = 0; i < n; ++i) std::copy(S_in + i * n, S_in + i * n + i + 1, m.begin() + i * ld);
  std::copy(rhs_in, rhs_in + n, m.begin() + n * ld);
  // a solve's steps overwrite y before they read it; other consumers of the
  // context (ITERATIVE_SCHUR) own it between calls: put it back afterwards
  std::vector<double> y_keep(n);
  HIP_OK(hipMemcpyAsync(y_keep.data(), W.y, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  double flags[2] = {0.0, 0.0};   // SL_CHOL_BAD, SL_CHOL_SPIN
  for (int attempt = 0;; ++attempt) {
    HIP_OK(hipMemcpyAsync(W.S, m.data(), sizeof(double) * m.size(), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(W.scal + SL_CHOL_BAD, 0, sizeof(double), s));
    HIP_OK(hipMemsetAsync(W.scal + SL_CHOL_SPIN, 0, sizeof(double), s));
    launch_cholesky_solve2(ctx->P, W, ++ctx->chol_epoch, s);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(&flags[0], W.scal + SL_CHOL_BAD, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(&flags[1], W.scal + SL_CHOL_SPIN, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (flags[1] == 0.0) break;
    // a hand-off of the factorisation never came: as in ba_covariance, once
    // more with the per-step launches (kept for this context)
    if (attempt > 0 || (!W.chol_persist && !W.chol_fuse && !W.chol_flow)) {
      HIP_OK(hipMemsetAsync(W.S, 0, sizeof(double) * m.size(), s));
      HIP_OK(hipMemsetAsync(W.scal + SL_CHOL_BAD, 0, sizeof(double), s));
      HIP_OK(hipMemsetAsync(W.scal + SL_CHOL_SPIN, 0, sizeof(double), s));
      HIP_OK(hipMemcpyAsync(W.y, y_keep.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
      HIP_OK(hipStreamSynchronize(s));
      throw BaError{BA_ERR_DEVICE, "dense Cholesky: a hand-off spin bound was hit"};
    }
    W.chol_persist = W.chol_flow = W.chol_fuse = false;
  }
  if (L) {
    HIP_OK(hipMemcpyAsync(L, W.Lf, sizeof(double) * (n + 1) * n, hipMemcpyDeviceToHost, s));   // (ld == n)
    HIP_OK(hipStreamSynchronize(s));
    // rows < n: the kernels store the tiles left of the diagonal 64-block
    // only; the rest of the buffer is stale
    for (size_t i = 0; i < n; ++i) std::fill(L + i * n + (i / 64) * 64, L + (i + 1) * n, 0.0);
    if (n % 64 == 0) {
      // the rhs row is a tile row of its own: no step factors it into z's
      // last block, k_back_flow forms z_K = V_K A_{n,K}^T in LDS from the
      // updated rhs row and stores nothing; the same product here (its
      // summation order: four strided partial sums, then their pairwise sum)
      const size_t K = T - 1;
      std::vector<double> a(64), v(64 * 64);
      HIP_OK(hipMemcpyAsync(a.data(), W.S + n * ld + K * 64, sizeof(double) * 64, hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(v.data(), W.Vbuf + K * 64 * 64, sizeof(double) * 64 * 64, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      for (size_t j = 0; j < 64; ++j) {
        double part[4];
        for (size_t h = 0; h < 4; ++h) {
          double t = 0.0;
          for (size_t q = 0; q < 16; ++q) {
            const size_t i = h + 4 * q;
            t = std::fma(i <= j ? v[j * 64 + i] : 0.0, a[i], t);
          }
          part[h] = t;
        }
        L[n * n + K * 64 + j] = (part[0] + part[1]) + (part[2] + part[3]);
      }
    }
  }
  if (V) HIP_OK(hipMemcpyAsync(V, W.Vbuf, sizeof(double) * T * 64 * 64, hipMemcpyDeviceToHost, s));
  if (y) HIP_OK(hipMemcpyAsync(y, W.y, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  // S held the updated trailing matrix: back to zeros, its state before the
  // first step (ensure_dense; the steps rely on its never-written blocks being
  // zero); the failure slots as a step's first kernels leave them
  HIP_OK(hipMemsetAsync(W.S, 0, sizeof(double) * m.size(), s));
  HIP_OK(hipMemsetAsync(W.scal + SL_CHOL_BAD, 0, sizeof(double), s));
  HIP_OK(hipMemsetAsync(W.scal + SL_CHOL_SPIN, 0, sizeof(double), s));
  HIP_OK(hipMemcpyAsync(W.y, y_keep.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
  HIP_OK(hipStreamSynchronize(s));
  if (ok) *ok = flags[0] == 0.0 ? 1 : 0;
}

}  // namespace

// ============================================================================
// extern "C" ABI
// ============================================================================
extern "C" {

int ba_abi_version(void) { return BA_ABI_VERSION; }

// ba_default_options: host/ba_options.cpp (plain C++, shared with the sanitizer build)

int ba_create(ba_ctx** out, int device) {
  if (!out) return BA_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  ba_ctx* ctx = new ba_ctx();
  try {
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) throw BaError{BA_ERR_INVALID_ARGUMENT, "invalid device " + std::to_string(device)};
    ctx->device = device;
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    for (auto& e : ctx->ev) HIP_OK(hipEventCreate(&e));
    {
      const size_t rec = sizeof(double) * (kNumSlots + kPcgState);
      HIP_OK(hipHostMalloc(&ctx->h_scal, rec + 64, hipHostMallocMapped | hipHostMallocCoherent));
      std::memset(ctx->h_scal, 0, rec + 64);
      ctx->h_seq = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(ctx->h_scal) + rec);
      void* d = nullptr;
      HIP_OK(hipHostGetDevicePointer(&d, ctx->h_scal, 0));
      ctx->d_hscal = static_cast<double*>(d);
      ctx->d_hseq = reinterpret_cast<unsigned*>(static_cast<char*>(d) + rec);
      HIP_OK(hipMalloc(&ctx->d_ticket, 64));
      HIP_OK(hipMemset(ctx->d_ticket, 0, 64));
    }
  } catch (const BaError& e) {
    std::fprintf(stderr, "ba_create: %s\n", e.msg.c_str());
    delete ctx;
    return e.code;
  }
  *out = ctx;
  return BA_OK;
}

int ba_destroy(ba_ctx* ctx) {
  if (!ctx) return BA_OK;
  (void)hipSetDevice(ctx->device);
  ctx->free_problem();
  if (ctx->comm) ncclCommDestroy(ctx->comm);
  for (auto& e : ctx->ev) if (e) (void)hipEventDestroy(e);
  if (ctx->h_scal) (void)hipHostFree(ctx->h_scal);
  if (ctx->d_ticket) (void)hipFree(ctx->d_ticket);
  if (ctx->hv_scratch) (void)hipFree(ctx->hv_scratch);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;   // (the staging arenas and the list buffers free their device memory here)
  return BA_OK;
}

const char* ba_last_error(const ba_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int ba_comm_unique_id(char id[128]) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  if (!id) return BA_ERR_INVALID_ARGUMENT;
  ncclUniqueId uid;
  if (ncclGetUniqueId(&uid) != ncclSuccess) return BA_ERR_COMM;
  std::memcpy(id, &uid, 128);
  return BA_OK;
}

int ba_comm_init(ba_ctx* ctx, const char id[128], int nranks, int rank) {
  if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    HIP_OK(hipSetDevice(ctx->device));
    if (ctx->comm) { ncclCommDestroy(ctx->comm); ctx->comm = nullptr; }
    ctx->host_fn = nullptr;
    ctx->nranks = nranks;
    ctx->rank = rank;
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    NCCL_OK(ncclCommInitRank(&ctx->comm, nranks, uid, rank));
    const char* fc = getenv("BA_FORCE_COLLECTIVES");
    ctx->force_coll = fc && atoi(fc) != 0;
  });
}

int ba_comm_allreduce_host(ba_ctx* ctx, double* values, int n, int op) {
  if (!ctx || n < 0 || (n > 0 && !values) || (op != 0 && op != 1)) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    if (!ctx->has_comm()) return;
    HIP_OK(hipSetDevice(ctx->device));
    double zero = 0.0;
    ctx->allreduce_host_values(n > 0 ? values : &zero, n > 0 ? (size_t)n : 1, op);   // n = 0: a barrier
  });
}

int ba_comm_init_host(ba_ctx* ctx, ba_host_allreduce_fn fn, void* user, int nranks, int rank) {
  if (!ctx || !fn || nranks < 1 || rank < 0 || rank >= nranks) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    if (ctx->comm) { ncclCommDestroy(ctx->comm); ctx->comm = nullptr; }
    ctx->host_fn = fn;
    ctx->host_user = user;
    ctx->nranks = nranks;
    ctx->rank = rank;
    const char* fc = getenv("BA_FORCE_COLLECTIVES");
    ctx->force_coll = fc && atoi(fc) != 0;
  });
}

int ba_set_problem(ba_ctx* ctx, const ba_problem* problem) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] { set_problem(ctx, problem); });
}

int ba_set_params(ba_ctx* ctx, const double* cams, const double* pts) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, "no problem"};
    if (cams && ctx->nc) HIP_OK(hipMemcpy(ctx->W.cams, cams, 6 * sizeof(double) * ctx->nc, hipMemcpyHostToDevice));
    if (pts && ctx->np) HIP_OK(hipMemcpy(ctx->W.pts, pts, 3 * sizeof(double) * ctx->np, hipMemcpyHostToDevice));
    // the Jacobi scaling belongs to the old parameters (ceres evaluates it at
    // the start of every solve): ba_bench_iterations must recompute it
    ctx->scale_valid = false;
  });
}

int ba_solve(ba_ctx* ctx, const ba_options* opt, ba_summary* summary) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] { HIP_OK(hipSetDevice(ctx->device)); solve(ctx, opt, summary); });
}

int ba_get_params(ba_ctx* ctx, double* cams, double* pts) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] { get_params(ctx, cams, pts); });
}

int ba_get_iteration_log(ba_ctx* ctx, ba_iteration* out, int n) {
  if (!ctx) return -BA_ERR_INVALID_ARGUMENT;
  const int avail = (int)ctx->log.size();
  if (out && n > 0) std::memcpy(out, ctx->log.data(), sizeof(ba_iteration) * std::min(n, avail));
  return avail;
}

int ba_eval_residuals(ba_ctx* ctx, double* r, double* cost) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, "no problem"};
    HIP_OK(hipSetDevice(ctx->device));
    const int no = ctx->no;
    double* d_r = nullptr;
    HIP_OK(hipMalloc(&d_r, sizeof(double) * 2 * std::max(no, 1)));
    DevFree guard{d_r};
    launch_cam_prep(ctx->P, ctx->W.cams, ctx->W.rec_c, false, ctx->stream);
    launch_residuals(ctx->P, ctx->W.rec_c, ctx->W.pts, d_r, ctx->stream);
    std::vector<double> rs(2 * (size_t)no);
    HIP_OK(hipMemcpyAsync(rs.data(), d_r, sizeof(double) * 2 * no, hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    double c = 0.0;
    const double a = ctx->huber_a, b = a * a;
    for (int s = 0; s < no; ++s) {
      const int o = ctx->perm[s];
      if (r) { r[2 * o] = rs[2 * s]; r[2 * o + 1] = rs[2 * s + 1]; }
      double sc;
      c += 0.5 * huber(rs[2 * s] * rs[2 * s] + rs[2 * s + 1] * rs[2 * s + 1], a, b, &sc);
    }
    if (cost) *cost = c;
  });
}

int ba_linearize(ba_ctx* ctx, double* r, double* J, double* cost) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, "no problem"};
    HIP_OK(hipSetDevice(ctx->device));
    ba_options o = options_or_default(nullptr);
    LinResult L = linearize(ctx, true, o.min_lm_diagonal, o.max_lm_diagonal);
    const int no = ctx->no;
    if (ctx->W.jrfree) {   // the iteration never stores J: write the records once for the read-back
      if (!ctx->W.JR) ctx->W.JR = ctx->dalloc<double>((size_t)(bahip::jr_ja_host(ctx->P.nc) + 8) * no);
      bahip::launch_linearize_jr(ctx->P, ctx->W, ctx->stream);
      // its cost partials are not this call's result (k_lin_point's were): fold
      // and clear them so no later reduction counts them
      launch_reduce(ctx->W, bit(SL_COST) | bit(SL_LIN_BAD), 0, ctx->stream);
      HIP_OK(hipStreamSynchronize(ctx->stream));
    }
    // record layout of ba_kernels.hip: JA [no][ja] (Jc rows; ja = 14: then r
    // again) then JB [no][8] (Jp rows, r)
    const int ja = bahip::jr_ja_host(ctx->P.nc);
    std::vector<double> rec((size_t)(ja + 8) * no);
    HIP_OK(hipMemcpy(rec.data(), ctx->W.JR, sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
    for (int s = 0; s < no; ++s) {
      const int o2 = ctx->perm[s];
      const double* qa = &rec[(size_t)s * ja];
      const double* qb = &rec[(size_t)ja * no + (size_t)s * 8];
      // bit patterns, not values: a NaN residual (zero depth) is still a
      // faithful copy of itself
      if (ja >= 14 && (std::memcmp(&qa[12], &qb[6], 2 * sizeof(double)) != 0))
        throw BaError{BA_ERR_DEVICE, "JR: the two residual copies differ"};
      if (r) { r[2 * o2] = qb[6]; r[2 * o2 + 1] = qb[7]; }
      if (J)
        for (int row = 0; row < 2; ++row) {
          for (int k = 0; k < 6; ++k) J[(size_t)o2 * 18 + row * 9 + k] = qa[row * 6 + k];
          for (int k = 0; k < 3; ++k) J[(size_t)o2 * 18 + row * 9 + 6 + k] = qb[row * 3 + k];
        }
    }
    if (cost) *cost = L.cost;
  });
}

int ba_debug_blocks(ba_ctx* ctx, double radius, double* Hpp, double* gp, double* Hcc, double* gc, double* S,
                    double* rhs, int* n_out) {
  if (!ctx || !(radius > 0.0)) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, "no problem"};
    HIP_OK(hipSetDevice(ctx->device));
    ba_options o = options_or_default(nullptr);   // DENSE_SCHUR, fp64
    ctx->read_env();
    // iteration 0's linearisation (Jacobi scaling from it), then the step's
    // reduced system without its factorisation
    const LinResult L = linearize(ctx, true, o.min_lm_diagonal, o.max_lm_diagonal);
    if (!L.ok) throw BaError{BA_ERR_DEVICE, "linearisation not finite"};
    step_w_storage(ctx, o);
    // BA_DEBUG_OV_PASS=1: S from the overlapped form's work items (a launch
    // that only forms S), else from the separate pair / diagonal / fold passes
    const char* dv = getenv("BA_DEBUG_OV_PASS");
    const bool want_ov = dv && dv[0] == '1';
    if (form_reduced_dense(ctx, radius, want_ov))
      launch_cholesky_solve_ov(ctx->P, ctx->W, ctx->W.ov, radius, ++ctx->chol_epoch, ctx->stream, true);
    else if (want_ov)
      throw BaError{BA_ERR_INVALID_ARGUMENT, "BA_DEBUG_OV_PASS: the overlapped form does not apply to this problem"};
    const hipStream_t st = ctx->stream;
    const int np = ctx->np, nc = ctx->nc, nvc = ctx->nvc, n = ctx->n;
    HIP_OK(hipStreamSynchronize(st));
    if (Hpp || gp) {
      std::vector<double> h(6 * (size_t)np), g(3 * (size_t)np);
      HIP_OK(hipMemcpy(h.data(), ctx->W.Hpp, h.size() * sizeof(double), hipMemcpyDeviceToHost));
      HIP_OK(hipMemcpy(g.data(), ctx->W.gp, g.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (int p = 0; p < np; ++p) {   // (SoA [k][np] on the device; fixed points: not written)
        const bool v = ctx->h_pt_var[p] != 0;
        for (int k = 0; k < 6; ++k) if (Hpp) Hpp[6 * (size_t)p + k] = v ? h[(size_t)k * np + p] : 0.0;
        for (int k = 0; k < 3; ++k) if (gp) gp[3 * (size_t)p + k] = v ? g[(size_t)k * np + p] : 0.0;
      }
    }
    if (Hcc || gc) {
      std::vector<double> h(27 * (size_t)std::max(nvc, 1));
      if (nvc) HIP_OK(hipMemcpy(h.data(), ctx->W.Hcc, 27 * (size_t)nvc * sizeof(double), hipMemcpyDeviceToHost));
      if (Hcc) std::fill(Hcc, Hcc + 21 * (size_t)nc, 0.0);
      if (gc) std::fill(gc, gc + 6 * (size_t)nc, 0.0);
      for (int v = 0; v < nvc; ++v) {
        const int c = ctx->cam_of_vc[v];
        for (int k = 0; k < 21; ++k) if (Hcc) Hcc[21 * (size_t)c + k] = h[21 * (size_t)v + k];
        for (int k = 0; k < 6; ++k) if (gc) gc[6 * (size_t)c + k] = h[21 * (size_t)nvc + 6 * (size_t)v + k];
      }
    }
    if (S || rhs) {
      std::vector<double> m((size_t)(n + 1) * std::max(ctx->ld, 1));
      if (n) HIP_OK(hipMemcpy(m.data(), ctx->W.S, m.size() * sizeof(double), hipMemcpyDeviceToHost));
      for (int i = 0; i < n; ++i) {
        if (S) for (int j = 0; j < n; ++j) S[(size_t)i * n + j] = j <= i ? m[(size_t)i * ctx->ld + j] : 0.0;
        if (rhs) rhs[i] = m[(size_t)n * ctx->ld + i];
      }
    }
    if (n_out) *n_out = n;
  });
}

int ba_debug_plan(ba_ctx* ctx, int32_t* out, int n) {
  if (!ctx || !out || n < 0) return BA_ERR_INVALID_ARGUMENT;
  if (!ctx->have_problem) return BA_ERR_NO_PROBLEM;
  // host state only (the order of include/ba_hip.h): nothing is built or launched
  const DevWork& W = ctx->W;
  const int32_t v[BA_DEBUG_PLAN_FIELDS] = {
      ctx->nvc, W.nblocks, W.neblocks, W.s_memset, ctx->have_dense && ctx->dup_diag, W.chol_persist, W.ov.ok,
      W.wcompact, W.jdiag, W.jrfree, ctx->have_dense, ctx->have_pcg, W.npchunks,
      ctx->have_pcg ? (int32_t)std::min<size_t>(ctx->pcg_ndup, INT32_MAX) : 0, W.pcgc, W.pacc, W.pcgjf};
  std::copy(v, v + std::min(n, (int)BA_DEBUG_PLAN_FIELDS), out);
  return BA_OK;
}

int ba_debug_factor(ba_ctx* ctx, const double* S_in, const double* rhs_in, double* L, double* V, double* y, int* ok) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] { debug_factor(ctx, S_in, rhs_in, L, V, y, ok); });
}

int ba_covariance_ex(ba_ctx* ctx, const ba_covariance_request_ex* req) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] { covariance(ctx, req, "ba_covariance_ex"); });
}

int ba_covariance(ba_ctx* ctx, const ba_covariance_request* req) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    if (!req) throw BaError{BA_ERR_INVALID_ARGUMENT, "ba_covariance: request is NULL"};
    ba_covariance_request_ex rx{};   // the same implementation, nothing else requested
    rx.base = *req;
    covariance(ctx, &rx, "ba_covariance");
  });
}

void ba_covariance_iterative_defaults(ba_cov_iter_options* opt) {
  if (!opt) return;
  opt->preconditioner_type = BA_SCHUR_JACOBI;
  opt->max_iterations = 500;
  opt->tolerance = 1e-10;
}

int ba_covariance_iterative(ba_ctx* ctx, const ba_covariance_request* req, const ba_cov_iter_options* opt,
                            ba_cov_iter_info* info) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] { covariance_iterative(ctx, req, opt, info); });
}

int ba_covariance_iterative_bench(ba_ctx* ctx, int cols, int reps, int warmup, double* ms) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] { covariance_iterative_bench(ctx, cols, reps, warmup, ms); });
}

int ba_covariance_times(ba_ctx* ctx, double* ms, int n) {
  return ctx ? copy_times(ctx->cov_ms, ms, n) : -BA_ERR_INVALID_ARGUMENT;
}

int ba_synchronize(ba_ctx* ctx) {
  if (!ctx) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] { HIP_OK(hipStreamSynchronize(ctx->stream)); });
}

int ba_bench_iteration_times(ba_ctx* ctx, double* ms, int n) {
  return ctx ? copy_times(ctx->bench_ms, ms, n) : BA_ERR_INVALID_ARGUMENT;   // (positive, unlike the other getters)
}

int ba_stream_copy(ba_ctx* ctx, size_t bytes, int reps, double* gbs) {
  if (!ctx || reps < 1 || bytes < 16 || !gbs) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    HIP_OK(hipSetDevice(ctx->device));
    const size_t n2 = bytes / 16;
    double *a = nullptr, *b = nullptr;
    HIP_OK(hipMalloc(&a, n2 * 16));
    DevFree free_a{a};
    if (hipMalloc(&b, n2 * 16) != hipSuccess) throw BaError{BA_ERR_OUT_OF_MEMORY, "ba_stream_copy: hipMalloc"};
    DevFree free_b{b};
    HIP_OK(hipMemsetAsync(a, 0, n2 * 16, ctx->stream));
    bahip::launch_stream_copy(a, b, n2, ctx->stream);   // warm-up
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(ctx->ev[0], ctx->stream));
    for (int r = 0; r < reps; ++r) bahip::launch_stream_copy(a, b, n2, ctx->stream);
    HIP_OK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIP_OK(hipEventSynchronize(ctx->ev[1]));
    float ms = 0.0f;
    HIP_OK(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    *gbs = 2.0 * 16.0 * (double)n2 * reps / ((double)ms * 1e-3) / 1e9;
  });
}

int ba_bench_iterations(ba_ctx* ctx, const ba_options* opt, int iters, double radius, double* ms_per_iter,
                        double* ms_rj_kernel, double* linear_iters) {
  if (!ctx || iters < 1) return BA_ERR_INVALID_ARGUMENT;
  return guarded(ctx, [&] {
    if (!ctx->have_problem) throw BaError{BA_ERR_NO_PROBLEM, "no problem"};
    HIP_OK(hipSetDevice(ctx->device));
    ba_options o = options_or_default(opt);
    check_options(o);
    ctx->clear_pending();
    if (!ctx->scale_valid) linearize(ctx, true, o.min_lm_diagonal, o.max_lm_diagonal);
    double rj_total = 0.0;
    long ls_total = 0;
    ctx->read_env();
    const bool spec = ctx->spec_lin;
    const bool trj = ms_rj_kernel != nullptr;   // event pair around the r+J kernel
    HIP_OK(hipEventRecord(ctx->ev[0], ctx->stream));
    ctx->rj_slot = 0;
    ctx->bench_ms.assign(iters, 0.0);
    double th = now_s();
    if (spec) linearize_enqueue(ctx, false, o.min_lm_diagonal, o.max_lm_diagonal, trj, true);
    for (int i = 0; i < iters; ++i) {
      // the solver's steady state after an accepted step: the step, its
      // scalar record, and the next linearisation (spec_lin_enqueue) behind
      // it while the host reads the record; K linearisations and K steps
      // (BA_SPEC_LIN=0: linearisation + step, then the read)
      const int slot = ctx->rj_slot;
      if (!spec) linearize_enqueue(ctx, false, o.min_lm_diagonal, o.max_lm_diagonal, trj, true);
      const int ls = step_enqueue(ctx, radius, o);
      ctx->publish_scalars();
      if (spec && i + 1 < iters) {
        ctx->rj_slot ^= 1;
        linearize_enqueue(ctx, false, o.min_lm_diagonal, o.max_lm_diagonal, trj, true);
      }
      ctx->wait_scalars();
      if (ctx->h_scal[SL_CHOL_SPIN] != 0.0) throw BaError{BA_ERR_DEVICE, "dense Cholesky: a hand-off spin bound was hit"};
      {   // (the iteration's record has arrived: its host wall time)
        const double t = now_s();
        ctx->bench_ms[i] = (t - th) * 1e3;
        th = t;
      }
      const StepResult st = step_result(ctx, ls);
      if (trj) {
        float rj = 0.0f;
        HIP_OK(hipEventSynchronize(ctx->ev[3 + 2 * slot]));
        HIP_OK(hipEventElapsedTime(&rj, ctx->ev[2 + 2 * slot], ctx->ev[3 + 2 * slot]));
        rj_total += rj;
      }
      ls_total += st.ls_iters;
    }
    HIP_OK(hipEventRecord(ctx->ev[1], ctx->stream));
    HIP_OK(hipEventSynchronize(ctx->ev[1]));
    float total = 0.0f;
    HIP_OK(hipEventElapsedTime(&total, ctx->ev[0], ctx->ev[1]));
    if (ms_per_iter) *ms_per_iter = total / iters;
    if (ms_rj_kernel) *ms_rj_kernel = rj_total / iters;
    if (linear_iters) *linear_iters = (double)ls_total / iters;
  });
}

}  // extern "C"
