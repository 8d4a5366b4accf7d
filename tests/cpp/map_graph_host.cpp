// map_graph_host.cpp — the host side of ba_map_graph compiled as a host
// program: the checker, the frame-sorted plan, the tile and chunk choice and
// the plain C++ restatement (check_map_table, map_graph_plan, map_graph_host:
// host/ba_batch_pack.hpp; the rules: csrc/ba_map_graph.h), run under ASan +
// UBSan by tests/test_map_graph_cpu.py.
//
// Input (the file named on the command line), mode "graph":
//   graph n_frames n_pts n_obs n_query have want_status table_reserved
//   th n_best order build_windows current_frame_id tile chunk reserved fraction
//   then the arrays whose bit is set in `have`, in this order (bit): frame_id (0), frame_is_key (1), pt_invalid (2),
//   pt_ref_frame (3), obs_offset (4, n_pts + 1 values), obs_frame (5), obs_octave (6), obs_outlier (7), query (8).
//   fraction is the hexadecimal bit pattern of the double.
// Output: "plan <tile> <chunk>", the frame offsets, the permutation, then per query "rec" + the ten fields, "W" + the raw
//   weight row, and the eight lists, one line each; with want_status a last line "status" + one value per point.
// A table the checker refuses prints "invalid <message>" and exits 0.
// Mode "synth" (for tools/map_graph_bench.py) reads "synth n_frames n_pts views n_query build_windows seed", draws the
// tracks itself and prints the seconds that plan and restatement took on this one thread.
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bundleadjustment_amd/csrc/ba_map_graph.h"
#include "../../bundleadjustment_amd/host/ba_batch_pack.hpp"

using namespace bahip;

static std::FILE* in;
static bool ok = true;

static std::vector<int32_t> ints(long n) {
  std::vector<int32_t> v((size_t)std::max(n, 0L));
  for (int32_t& x : v) ok = ok && std::fscanf(in, "%" SCNd32, &x) == 1;
  return v;
}
static std::vector<uint8_t> bytes(long n) {
  std::vector<int32_t> v = ints(n);
  return std::vector<uint8_t>(v.begin(), v.end());
}
static int one_int() { return ints(1)[0]; }
template <class V> static void line(const char* tag, const V& v, size_t first, size_t count) {
  std::printf("%s", tag);
  for (size_t i = 0; i < count; ++i) std::printf(" %d", (int)v[first + i]);
  std::printf("\n");
}

static int run_graph() {
  ba_map_table t{};
  t.n_frames = one_int(); t.n_pts = one_int(); t.n_obs = one_int();
  const int nq = one_int(), have = one_int(), want_status = one_int();
  t.reserved = one_int();
  ba_graph_options p{};
  p.th = one_int(); p.n_best = one_int(); p.order = one_int(); p.build_windows = one_int(); p.current_frame_id = one_int();
  p.debug_tile_frames = one_int(); p.debug_chunk_queries = one_int(); p.reserved = one_int();
  uint64_t fbits = 0;
  ok = ok && std::fscanf(in, "%" SCNx64, &fbits) == 1;
  std::memcpy(&p.redundant_fraction, &fbits, sizeof fbits);
  auto has = [&](int bit) { return (have >> bit) & 1; };
  const std::vector<int32_t> frame_id = ints(has(0) ? t.n_frames : 0);
  const std::vector<uint8_t> is_key = bytes(has(1) ? t.n_frames : 0), invalid = bytes(has(2) ? t.n_pts : 0);
  const std::vector<int32_t> ref = ints(has(3) ? t.n_pts : 0), off = ints(has(4) ? (long)t.n_pts + 1 : 0),
                             frame = ints(has(5) ? t.n_obs : 0), octave = ints(has(6) ? t.n_obs : 0);
  const std::vector<uint8_t> outlier = bytes(has(7) ? t.n_obs : 0);
  const std::vector<int32_t> query = ints(has(8) ? nq : 0);
  if (!ok) { std::fprintf(stderr, "short input\n"); return 2; }
  // a missing array is a null pointer, also where its length would be 0
  if (has(0)) t.frame_id = frame_id.data();
  if (has(1)) t.frame_is_key = is_key.data();
  if (has(2)) t.pt_invalid = invalid.data();
  if (has(3)) t.pt_ref_frame = ref.data();
  if (has(4)) t.obs_offset = off.data();
  if (has(5)) t.obs_frame = frame.data();
  if (has(6)) t.obs_octave = octave.data();
  if (has(7)) t.obs_outlier = outlier.data();
  try {
    const ba_graph_options o = check_map_table("map_graph_host: ", &t, has(8) ? query.data() : nullptr, nq, &p, want_status != 0);
    const MapGraphPlan M = map_graph_plan(&t);
    std::printf("plan %d %d\n", map_graph_tile(o, t.n_frames), map_graph_chunk(o, &t, nq));
    line("frame_off", M.frame_off, 0, M.frame_off.size());
    line("perm", M.perm, 0, M.perm.size());
    const MapGraphHost R = map_graph_host(&t, M, query.data(), nq, o, want_status != 0);
    size_t at[4] = {0, 0, 0, 0};
    std::vector<int32_t> W;
    for (int i = 0; i < nq; ++i) {
      const ba_graph_frame& r = R.rec[(size_t)i];
      std::printf("rec %d %d %d %d %d %d %d %d %d %d\n", r.status, r.degree, r.max_weight, r.n_map, r.n_redundant, r.cull,
                  r.n_local, r.n_fixed, r.n_win_pts, r.n_win_obs);
      map_graph_host_weights(&t, M, query[(size_t)i], W);
      line("W", W, 0, W.size());
      const size_t nc = (size_t)(r.n_local + r.n_fixed);
      line("nbr_frame", R.nbr_frame, at[0], (size_t)r.degree); line("nbr_weight", R.nbr_weight, at[0], (size_t)r.degree);
      line("win_cam", R.win_cam, at[1], nc); line("win_cam_fixed", R.win_cam_fixed, at[1], nc);
      line("win_pt", R.win_pt, at[2], (size_t)r.n_win_pts);
      line("win_obs", R.win_obs, at[3], (size_t)r.n_win_obs); line("win_obs_cam", R.win_obs_cam, at[3], (size_t)r.n_win_obs);
      line("win_obs_pt", R.win_obs_pt, at[3], (size_t)r.n_win_obs);
      at[0] += (size_t)r.degree; at[1] += nc; at[2] += (size_t)r.n_win_pts; at[3] += (size_t)r.n_win_obs;
    }
    if (want_status) line("status", R.pt_status, 0, R.pt_status.size());
  } catch (const BaError& e) {
    std::printf("invalid %s\n", e.msg.c_str());
  }
  return 0;
}

static int run_synth() {
  const int nf = one_int(), np = one_int(), views = one_int(), nq = one_int(), windows = one_int();
  uint64_t s = (uint64_t)one_int() * 0x9E3779B97F4A7C15ull + 1;
  if (!ok || nf < views || views < 1) { std::fprintf(stderr, "bad synth line\n"); return 2; }
  auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  std::vector<int32_t> frame_id((size_t)nf), off((size_t)np + 1), frame((size_t)np * views), query((size_t)nq);
  for (int f = 0; f < nf; ++f) frame_id[(size_t)f] = f;
  for (int q = 0; q < nq; ++q) query[(size_t)q] = (int32_t)((int64_t)q * nf / nq);
  for (int p = 0; p < np; ++p) {       // a window of 2 * views consecutive frames, `views` of them at a stride of 2
    off[(size_t)p + 1] = (p + 1) * views;
    const int f0 = (int)(next() % (uint64_t)nf);
    for (int k = 0; k < views; ++k) frame[(size_t)p * views + k] = (f0 + 2 * k + (int)(next() & 1)) % nf;
  }
  ba_map_table t{};
  t.n_frames = nf; t.n_pts = np; t.n_obs = np * views;
  t.frame_id = frame_id.data(); t.obs_offset = off.data(); t.obs_frame = frame.data();
  ba_graph_options o;
  map_graph_defaults(o);
  o.build_windows = windows;
  const auto t0 = std::chrono::steady_clock::now();
  const MapGraphPlan M = map_graph_plan(&t);
  const MapGraphHost R = map_graph_host(&t, M, query.data(), nq, o, false);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  long long sum = 0;
  for (const ba_graph_frame& r : R.rec) sum += r.degree + r.n_win_obs;
  std::printf("%.6f %lld\n", sec, sum);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2 || !(in = std::fopen(argv[1], "r"))) { std::fprintf(stderr, "usage: map_graph_host <case file>\n"); return 2; }
  char mode[16] = {0};
  if (std::fscanf(in, "%15s", mode) != 1) return 2;
  const int rc = !std::strcmp(mode, "graph") ? run_graph() : !std::strcmp(mode, "synth") ? run_synth() : 2;
  std::fclose(in);
  return rc;
}
