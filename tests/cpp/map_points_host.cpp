// map_points_host.cpp — the pinned arithmetic of ba_map_points_update and
// ba_associate (bundleadjustment_amd/csrc/ba_map_points.h) and their host-side
// checking and planning (check_map_points, map_points_plan, check_assoc:
// host/ba_batch_pack.hpp) compiled as a host program, run under ASan + UBSan by
// tests/test_map_points_cpu.py (built with -ffp-contract=off, as the header
// asks).  It walks a batch serially the way the kernels do: norms first, one
// row of D at a time, the row median by counting the keys before each key (up
// to 64 observations, as the lane groups do) and digit by digit from counts
// (every length, as the workgroup route does); the two must agree.  Floats
// travel as the hexadecimal bit patterns of their float32 values.
//
// Input (the file named on the command line), mode "mp":
//   mp dim n_cams n_pts n_rows n_obs have_scale have_ref median_rule reserved max_scale reserved_f
//   cam_center[3 n_cams] pts[3 n_pts] obs_offset[n_pts + 1] obs_cam[n_obs] obs_row[n_obs]
//   have_scale: obs_scale[n_obs]   have_ref: ref_obs[n_pts]   desc[n_rows * dim]
// Output: "plan <first0> <count0> <first1> <count1> <first2> <count2> <layout bytes>", then per point
//   "point <p> <n> <status> <best> <median> <v0> <v1> <v2> <min> <max>", n lines of D, one line of m.
// Mode "assoc":
//   assoc dim n_cams n_pts n_rows n_items n_fuse have_scale have_cur chi2 min_cos max_desc fuse_min_cos fuse_max_desc reserved
//   extr cam_center K image_size pts pt_view_dir pt_dist pt_desc desc item_cam item_pt item_uv [item_scale]
//   item_row [item_cur_row] fuse_pairs
// Output: n_items lines "status chi cosine world_dist dist_matched dist_current", n_fuse lines "status cosine dist".
// With the word "time" as a second argument the mp mode prints only the
// seconds that the points took.  Mode "synth" (for tools/map_points_bench.py)
// reads "synth dim n_pts views n_rows seed", draws unit-norm rows and tracks
// itself and prints the seconds that the points took on this one thread.
// A batch the checker refuses prints "invalid <message>" and exits 0.
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bundleadjustment_amd/csrc/ba_map_points.h"
#include "../../bundleadjustment_amd/host/ba_batch_pack.hpp"

using namespace bahip;

static std::FILE* in;
static bool ok = true;

static std::vector<float> floats(size_t n) {
  std::vector<float> v(n);
  for (float& x : v) {
    uint32_t u = 0;
    ok = ok && std::fscanf(in, "%" SCNx32, &u) == 1;
    x = match_float(u);
  }
  return v;
}
static std::vector<int32_t> ints(size_t n) {
  std::vector<int32_t> v(n);
  for (int32_t& x : v) ok = ok && std::fscanf(in, "%" SCNd32, &x) == 1;
  return v;
}
static float one_float() { return floats(1)[0]; }
static int one_int() { return ints(1)[0]; }
static void put(float v) { std::printf(" %08" PRIx32, match_bits(v)); }

struct PointResult { ba_map_point rec; std::vector<float> D, m; };

static PointResult run_point(const ba_map_point_batch& b, const ba_map_point_options& p, int q, bool keep) {
  PointResult R;
  const int dim = b.dim, o0 = b.obs_offset[q], n = b.obs_offset[q + 1] - o0, k = mp_rank(n);
  ba_map_point& r = R.rec;
  std::memset(&r, 0, sizeof r);
  if (n == 0) { r.status = BA_MP_EMPTY; r.best = -1; return R; }
  std::vector<float> nrm((size_t)n), row((size_t)n);
  R.m.resize((size_t)n);
  if (keep) R.D.resize((size_t)n * n);
  auto desc = [&](int i) { return b.desc + (size_t)b.obs_row[o0 + i] * dim; };
  for (int i = 0; i < n; ++i) nrm[(size_t)i] = match_dot(desc(i), desc(i), dim);
  uint64_t best = ~0ull;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) row[(size_t)j] = mp_distance(desc(i), desc(j), nrm[(size_t)i], nrm[(size_t)j], dim);
    const uint32_t mb = mp_select_bits(k, [&](uint32_t x) {
      int c = 0;
      for (int j = 0; j < n; ++j) c += match_bits(row[(size_t)j]) < x ? 1 : 0;
      return c;
    });
    if (n <= kMpWave) {   // the lane groups' way: the key with exactly k keys before it
      int hits = 0;
      for (int j = 0; j < n; ++j) {
        int before = 0;
        for (int t = 0; t < n; ++t) before += mp_key_before(match_bits(row[(size_t)t]), t, match_bits(row[(size_t)j]), j) ? 1 : 0;
        if (before == k) { ++hits; if (match_bits(row[(size_t)j]) != mb) { std::fprintf(stderr, "the two selections differ\n"); std::exit(5); } }
      }
      if (hits != 1) { std::fprintf(stderr, "%d keys of rank k\n", hits); std::exit(5); }
    }
    R.m[(size_t)i] = match_float(mb);
    if (keep) std::memcpy(&R.D[(size_t)i * n], row.data(), sizeof(float) * (size_t)n);
    best = std::min(best, mp_choice_key(R.m[(size_t)i], i, p.median_rule));
  }
  r.status = BA_MP_OK; r.best = (int32_t)(uint32_t)best; r.median = R.m[(size_t)r.best];
  float s[3] = {0.0f, 0.0f, 0.0f};
  for (int t = 0; t < n; ++t) {
    float u[3];
    mp_view_unit(b.cam_center + 3 * (size_t)b.obs_cam[o0 + t], b.pts + 3 * (size_t)q, u);
    for (int c = 0; c < 3; ++c) s[c] = mp_add(s[c], u[c]);
  }
  for (int c = 0; c < 3; ++c) r.view_dir[c] = mp_div(s[c], (float)n);
  const int ref = b.ref_obs ? b.ref_obs[q] : 0;
  mp_depth_bounds(b.cam_center + 3 * (size_t)b.obs_cam[o0 + ref], b.pts + 3 * (size_t)q, b.obs_scale ? b.obs_scale[o0 + ref] : 1.0f,
                  p.max_scale, r.min_dist, r.max_dist);
  return R;
}

static int run_mp(bool time_only) {
  ba_map_point_batch b{};
  ba_map_point_options opt{};
  b.dim = one_int(); b.n_cams = one_int(); b.n_pts = one_int(); b.n_rows = one_int();
  const int n_obs = one_int(), have_scale = one_int(), have_ref = one_int();
  opt.median_rule = one_int(); opt.reserved = one_int(); opt.max_scale = one_float(); opt.reserved_f = one_float();
  if (!ok || b.dim <= 0 || b.n_cams < 0 || b.n_pts < 0 || b.n_rows < 0 || n_obs < 0) { std::fprintf(stderr, "bad case file\n"); return 3; }
  // (the arrays are sized by the declared counts: they cover the indices of every case, refused ones included)
  const std::vector<float> center = floats(3 * (size_t)b.n_cams), pts = floats(3 * (size_t)b.n_pts);
  const std::vector<int32_t> off = ints((size_t)b.n_pts + 1), cam = ints((size_t)n_obs), row = ints((size_t)n_obs);
  const std::vector<float> scale = floats(have_scale ? (size_t)n_obs : 0);
  const std::vector<int32_t> ref = ints(have_ref ? (size_t)b.n_pts : 0);
  const std::vector<float> desc = floats((size_t)b.n_rows * (size_t)b.dim);
  if (!ok || off.back() > n_obs) { std::fprintf(stderr, "bad case file\n"); return 3; }
  b.cam_center = center.data(); b.pts = pts.data(); b.obs_offset = off.data(); b.obs_cam = cam.data(); b.obs_row = row.data();
  b.obs_scale = have_scale ? scale.data() : nullptr; b.ref_obs = have_ref ? ref.data() : nullptr; b.desc = desc.data();
  ba_map_point_options p;
  try {
    p = check_map_points("map_points_host: ", &b, &opt);
  } catch (const BaError& e) {
    std::printf("invalid %s\n", e.msg.c_str());
    return 0;
  }
  if (time_only) {
    const auto t0 = std::chrono::steady_clock::now();
    int sum = 0;
    for (int q = 0; q < b.n_pts; ++q) sum += run_point(b, p, q, false).rec.best;
    std::printf("%.6f %d\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), sum);
    return 0;
  }
  const MapPointsPlan M = map_points_plan(&b, 0, b.n_pts);
  const MapPointsLayout L = map_points_layout(&b, (size_t)b.n_pts, true, 0);
  std::printf("plan %d %d %d %d %d %d %zu\n", M.first[0], M.count[0], M.first[1], M.count[1], M.first[2], M.count[2], L.L.total);
  std::vector<char> seen((size_t)b.n_pts, 0);
  for (int t = 0; t < 3; ++t)
    for (int s = 0; s < M.count[t]; ++s) {
      const int q = M.order[(size_t)(M.first[t] + s)];
      if (q < 0 || q >= b.n_pts || seen[(size_t)q] || map_points_tier(off[(size_t)q + 1] - off[(size_t)q]) != t) {
        std::fprintf(stderr, "bad plan\n");
        return 4;
      }
      seen[(size_t)q] = 1;
    }
  for (int q = 0; q < b.n_pts; ++q) {
    const PointResult R = run_point(b, p, q, true);
    const int n = (int)R.m.size();
    std::printf("point %d %d %d %d", q, n, R.rec.status, R.rec.best);
    put(R.rec.median); put(R.rec.view_dir[0]); put(R.rec.view_dir[1]); put(R.rec.view_dir[2]); put(R.rec.min_dist); put(R.rec.max_dist);
    std::printf("\n");
    for (int i = 0; i < n; ++i) {
      for (int j = 0; j < n; ++j) put(R.D[(size_t)i * n + j]);
      std::printf("\n");
    }
    for (int i = 0; i < n; ++i) put(R.m[(size_t)i]);
    std::printf("\n");
  }
  return 0;
}

static int run_assoc() {
  ba_assoc_batch b{};
  ba_assoc_options opt{};
  b.dim = one_int(); b.n_cams = one_int(); b.n_pts = one_int(); b.n_rows = one_int(); b.n_items = one_int(); b.n_fuse = one_int();
  const int have_scale = one_int(), have_cur = one_int();
  opt.chi2 = one_float(); opt.min_cos = one_float(); opt.max_desc_dist = one_float(); opt.fuse_min_cos = one_float();
  opt.fuse_max_desc_dist = one_float(); opt.reserved = one_int();
  if (!ok || b.dim <= 0 || b.n_cams < 0 || b.n_pts < 0 || b.n_rows < 0 || b.n_items < 0 || b.n_fuse < 0) { std::fprintf(stderr, "bad case file\n"); return 3; }
  const size_t nc = (size_t)b.n_cams, np = (size_t)b.n_pts, ni = (size_t)b.n_items, nf = (size_t)b.n_fuse, dim = (size_t)b.dim;
  const std::vector<float> extr = floats(16 * nc), center = floats(3 * nc), K = floats(9 * nc);
  const std::vector<int32_t> size = ints(2 * nc);
  const std::vector<float> pts = floats(3 * np), dir = floats(3 * np), dist = floats(2 * np), pdesc = floats(np * dim),
                           desc = floats((size_t)b.n_rows * dim);
  const std::vector<int32_t> icam = ints(ni), ipt = ints(ni);
  const std::vector<float> uv = floats(2 * ni), scale = floats(have_scale ? ni : 0);
  const std::vector<int32_t> irow = ints(ni), cur = ints(have_cur ? ni : 0), fuse = ints(2 * nf);
  if (!ok) { std::fprintf(stderr, "bad case file\n"); return 3; }
  b.extr = extr.data(); b.cam_center = center.data(); b.K = K.data(); b.image_size = size.data(); b.pts = pts.data();
  b.pt_view_dir = dir.data(); b.pt_dist = dist.data(); b.pt_desc = pdesc.data(); b.desc = desc.data();
  b.item_cam = icam.data(); b.item_pt = ipt.data(); b.item_uv = uv.data(); b.item_scale = have_scale ? scale.data() : nullptr;
  b.item_row = irow.data(); b.item_cur_row = have_cur ? cur.data() : nullptr; b.fuse_pairs = fuse.data();
  ba_assoc_options p;
  try {
    p = check_assoc("map_points_host: ", &b, &opt);
  } catch (const BaError& e) {
    std::printf("invalid %s\n", e.msg.c_str());
    return 0;
  }
  (void)assoc_layout(&b);
  for (size_t t = 0; t < ni; ++t) {
    const size_t c = (size_t)icam[t], q = (size_t)ipt[t];
    const int cr = have_cur ? cur[t] : -1;
    const ba_assoc_result r =
        mp_associate(&extr[16 * c], &center[3 * c], &K[9 * c], size[2 * c], size[2 * c + 1], &pts[3 * q], &dir[3 * q], &dist[2 * q],
                     &uv[2 * t], have_scale ? scale[t] : 1.0f, &desc[dim * (size_t)irow[t]],
                     cr >= 0 ? &desc[dim * (size_t)cr] : nullptr, &pdesc[dim * q], b.dim, p);
    std::printf("%d", r.status);
    put(r.chi); put(r.cosine); put(r.world_dist); put(r.dist_matched); put(r.dist_current);
    std::printf("\n");
  }
  for (size_t f = 0; f < nf; ++f) {
    const size_t a = (size_t)fuse[2 * f], c = (size_t)fuse[2 * f + 1];
    const ba_fuse_result r = mp_fuse(&dir[3 * a], &dir[3 * c], &pdesc[dim * a], &pdesc[dim * c], b.dim, p);
    std::printf("%d", r.status);
    put(r.cosine); put(r.dist);
    std::printf("\n");
  }
  return 0;
}

static int run_synth() {
  const int dim = one_int(), n_pts = one_int(), views = one_int(), n_rows = one_int();
  uint64_t state = (uint64_t)one_int() * 2862933555777941757ull + 3037000493ull;
  if (!ok || (dim != 64 && dim != 128) || n_pts < 0 || views < 1 || views > BA_MP_MAX_TRACK || n_rows < 1) {
    std::fprintf(stderr, "bad case file\n");
    return 3;
  }
  auto next = [&] { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
  std::vector<float> desc((size_t)n_rows * (size_t)dim), center(3 * 16), pts(3 * (size_t)n_pts);
  for (size_t r = 0; r < (size_t)n_rows; ++r) {
    double nrm = 0.0;
    for (int k = 0; k < dim; ++k) { const float v = (float)next() / 1073741824.0f - 1.0f; desc[r * dim + k] = v; nrm += (double)v * v; }
    for (int k = 0; k < dim; ++k) desc[r * dim + k] = (float)(desc[r * dim + k] / std::sqrt(nrm > 0 ? nrm : 1.0));
  }
  for (float& v : center) v = (float)next() / 1073741824.0f - 1.0f;
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = (float)next() / 1073741824.0f - 1.0f + (i % 3 == 2 ? 6.0f : 0.0f);
  std::vector<int32_t> off((size_t)n_pts + 1), cam((size_t)n_pts * views), row((size_t)n_pts * views);
  for (int q = 0; q <= n_pts; ++q) off[(size_t)q] = q * views;
  for (size_t o = 0; o < cam.size(); ++o) { cam[o] = (int32_t)(next() % 16); row[o] = (int32_t)(next() % (uint32_t)n_rows); }
  ba_map_point_batch b{};
  b.dim = dim; b.n_cams = 16; b.n_pts = n_pts; b.n_rows = n_rows;
  b.cam_center = center.data(); b.pts = pts.data(); b.obs_offset = off.data(); b.obs_cam = cam.data(); b.obs_row = row.data();
  b.desc = desc.data();
  const ba_map_point_options p = check_map_points("map_points_host: ", &b, nullptr);
  const auto t0 = std::chrono::steady_clock::now();
  long long sum = 0;
  for (int q = 0; q < n_pts; ++q) sum += run_point(b, p, q, false).rec.best;
  std::printf("%.6f %lld\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), sum);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) { std::fprintf(stderr, "usage: map_points_host <case> [time]\n"); return 2; }
  in = std::fopen(argv[1], "r");
  if (!in) { std::perror(argv[1]); return 2; }
  char mode[16] = {0};
  if (std::fscanf(in, "%15s", mode) != 1) { std::fprintf(stderr, "bad case file\n"); return 3; }
  const int rc = std::strcmp(mode, "mp") == 0 ? run_mp(argc == 3 && std::strcmp(argv[2], "time") == 0)
               : std::strcmp(mode, "assoc") == 0 ? run_assoc()
               : std::strcmp(mode, "synth") == 0 ? run_synth() : 3;
  std::fclose(in);
  return rc;
}
