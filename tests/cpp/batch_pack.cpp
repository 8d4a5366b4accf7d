// batch_pack.cpp — the host-only packer of the batch entry points
// (bundleadjustment_amd/host/ba_batch_pack.hpp) as a stand-alone program:
// the section layout, check_offsets, and the structure build of
// ba_solve_window_batch on a batch read from a file.  Built with ASan + UBSan
// by `make sanitize` (tests/test_sanitize.py writes the batch and checks every
// output array).
//
// in.bin:  int32 n, NC, NP, NO, flags (1: cam_fixed, 2: pt_fixed); int32
//          cam_offset[n+1], pt_offset[n+1], obs_offset[n+1]; [u8 cam_fixed[NC]];
//          [u8 pt_fixed[NP]]; int32 obs_cam[NO], obs_pt[NO]; f32 obs_uv[2 NO].
//          Every array is held in a heap block of exactly its size.
// out.bin: prob, cam_vc, pt_var, pt_off, obs_cam, obs_slot, uv, cam_off,
//          cam_obs, NV, each as int64 byte count + bytes.
// Exit status 3 + the message on stdout when the packer refuses the batch.
//
// `batch_pack_san check NAME` runs instead one validator of the other entry
// points (ba_prune, ba_solve_pose_batch, ba_triangulate, the window log
// capacity, the hypothesis range of the inspection entries) on one accepted or
// one refused batch, or with NAME = layouts every layout builder: sections
// aligned, not overlapping, in_b <= io_b <= total.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <vector>

#include "ba_batch_pack.hpp"

using namespace bahip;

template <class T>
static std::vector<T> get(std::ifstream& f, size_t n) {
  std::vector<T> v(n);
  f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(n * sizeof(T)));
  if (!f) throw std::runtime_error("short input file");
  return v;
}
template <class T>
static void put(std::ofstream& f, const std::vector<T>& v) {
  const int64_t nb = static_cast<int64_t>(v.size() * sizeof(T));
  f.write(reinterpret_cast<const char*>(&nb), sizeof nb);
  f.write(reinterpret_cast<const char*>(v.data()), nb);
}

static void offsets_message(const std::vector<int32_t>& off, const char* unit) {
  try {
    check_offsets("fn: ", "off", off.data(), (int)off.size() - 1, unit);
    std::printf("offsets ok\n");
  } catch (const BaError& e) {
    std::printf("offsets %d %s\n", e.code, e.msg.c_str());
  }
}

// ---------------------------------------------------------------------------
// `batch_pack_san check NAME`: one validator on one batch (exit 0 and "ok", or
// exit 3 and the refusal), or, NAME = layouts, every layout builder.  Every
// array is a vector of exactly its size, so a read past its end is a finding.
// ---------------------------------------------------------------------------
struct Section { size_t off, bytes; };

// the sections in layout order: aligned, not overlapping, inputs before in_b,
// outputs before io_b, everything before total
static void check_sections(const char* name, const SectionLayout& L, size_t align, const std::vector<Section>& in,
                           const std::vector<Section>& out, const std::vector<Section>& scratch) {
  auto fail = [&](const char* what) { throw std::runtime_error(std::string(name) + ": " + what); };
  if (!(L.in_b <= L.io_b && L.io_b <= L.total)) fail("in_b <= io_b <= total does not hold");
  size_t at = 0;
  const std::vector<Section>* groups[3] = {&in, &out, &scratch};
  const size_t end[3] = {L.in_b, L.io_b, L.total};
  for (int g = 0; g < 3; ++g) {
    for (const Section& s : *groups[g]) {
      if (s.off % align) fail("a section is not aligned");
      if (s.off < at) fail("two sections overlap");
      at = s.off + s.bytes;
      if (at > end[g]) fail("a section passes the end of its group");
    }
    at = end[g];
  }
  if (L.in_b % align || L.io_b % align || L.total % align) fail("a group end is not aligned");
  std::printf("layout %s: %zu %zu %zu\n", name, L.in_b, L.io_b, L.total);
}

static void check_layouts() {
  {
    const size_t NC = 3, NO = 7;
    const PruneLayout P = prune_layout(NC, NO);
    check_sections("prune", P.L, 1, {{P.extr, 64 * NC}, {P.ctr, 12 * NC}, {P.K, 36 * NC}, {P.X, 12 * NO}, {P.uv, 8 * NO},
                                     {P.sig, 4 * NO}, {P.dist, 8 * NO}, {P.cam, 4 * NO}}, {{P.res, NO}}, {});
  }
  {
    const size_t N = 3, NO = 11;
    const PoseLayout P = pose_layout(N, NO);
    check_sections("pose", P.L, 16, {{P.off, 4 * (N + 1)}, {P.cam, 48 * N}, {P.K, 36 * N}, {P.X, 24 * NO}, {P.uv, 8 * NO}},
                   {{P.out, 48 * N}, {P.summ, 64 * N}}, {});
  }
  for (int opt = 0; opt < 8; ++opt) {
    const size_t nc = 5, np = 9, no = 31;
    const bool ctr = opt & 1, sc = opt & 2, given = opt & 4;
    const TriLayout P = tri_layout(nc, np, no, ctr, sc, given);
    check_sections("tri", P.L, 256, {{P.extr, 64 * nc}, {P.ctr, ctr ? 12 * nc : 0}, {P.K, 36 * nc}, {P.off, 4 * (np + 1)},
                                     {P.oc, 4 * no}, {P.uv, 8 * no}, {P.sc, sc ? 4 * no : 0}, {P.init, given ? 24 * np : 0}},
                   {{P.pts, 24 * np}, {P.summ, 48 * np}, {P.st, np}}, {{P.rec, 8 * (size_t)kTriRec * nc}});
  }
  {
    WindowPack w;
    const size_t n = 2, NC = 5, NP = 9, NO = 31, log_cap = 51;
    w.prob.resize(n); w.cam_vc.resize(NC); w.pt_var.resize(NP); w.pt_off.resize(NP + n); w.obs_cam.resize(NO);
    w.obs_slot.resize(NO); w.uv.resize(2 * NO); w.cam_off.resize(6); w.cam_obs.resize(27); w.NV = 4;
    const WindowLayout P = window_layout(w, log_cap);
    check_sections("window", P.L, 256,
                   {{P.prob, sizeof(WinProb) * n}, {P.cams, 48 * NC}, {P.pts, 24 * NP}, {P.K, 36 * NC}, {P.extr, 64 * NC},
                    {P.vc, 4 * NC}, {P.pv, NP}, {P.poff, 4 * (NP + n)}, {P.oc, 4 * NO}, {P.slot, 4 * NO}, {P.uv, 8 * NO},
                    {P.coff, 4 * 6}, {P.cobs, 4 * 27}},
                   {{P.cams_out, 48 * NC}, {P.pts_out, 24 * NP}, {P.summ, 64 * n}, {P.log, sizeof(ba_iteration) * log_cap * n}},
                   {{P.w_pts, 48 * NP}, {P.w_ctab, 16 * (size_t)kWinTbl * NC}, {P.w_vrec, 8 * (size_t)kWinVRec * NC},
                    {P.w_JR, 16 * (size_t)kWinJR * NO}, {P.w_Hp, 144 * NP}, {P.w_sp, 24 * NP}, {P.w_prec, 72 * NP},
                    {P.w_W, 144 * NO}, {P.w_hc, 432 * w.NV}});
  }
  for (int opt = 0; opt < 4; ++opt) {
    const bool status = opt & 1, windows = opt & 2;
    const std::vector<int32_t> frame_id(40), off(101), frame(333), octave(333);
    const std::vector<uint8_t> is_key(40), outlier(333);
    ba_map_table t{};
    t.n_frames = 40; t.n_pts = 100; t.n_obs = 333;
    t.frame_id = frame_id.data(); t.obs_offset = off.data(); t.obs_frame = frame.data();
    t.frame_is_key = windows ? is_key.data() : nullptr; t.obs_octave = status ? octave.data() : nullptr;
    t.obs_outlier = windows ? nullptr : outlier.data();
    ba_graph_options p;
    map_graph_defaults(p);
    p.build_windows = windows;
    const size_t nf = 40, np = 100, no = 333, nq = 7, nc = 3, fw = map_graph_words(40), pw = windows ? map_graph_words(100) : 0;
    const MapGraphLayout P = map_graph_layout(&t, p, (int)nq, (int)nc, status);
    check_sections("map_graph", P.L, 256,
                   {{P.frame_id, 4 * nf}, {P.is_key, windows ? nf : 0}, {P.pt_invalid, 0}, {P.pt_ref, status ? 4 * np : 0},
                    {P.off, 4 * (np + 1)}, {P.frame, 4 * no}, {P.octave, status ? 4 * no : 0}, {P.outlier, windows ? 0 : no},
                    {P.obs_pt, 4 * no}, {P.perm, 4 * no}, {P.frame_off, 4 * (nf + 1)}, {P.query, 4 * nq}},
                   {{P.rec, sizeof(ba_graph_frame) * nq}, {P.status, status ? np : 0}},
                   {{P.W, 4 * nc * nf}, {P.lst_f, 4 * nc * nf}, {P.lst_w, 4 * nc * nf}, {P.best, 4 * nc * BA_WINDOW_MAX_CAMS},
                    {P.loc, 4 * nc * fw}, {P.fix, 4 * nc * fw}, {P.pre, 4 * nc * fw}, {P.ptb, 4 * nc * pw}, {P.offs, 32 * nc}});
  }
}

// NAME = <entry>[_<mutation>]: the accepted batch of the entry, or that batch with one thing wrong
static int check_case(const std::string& name) {
  auto is = [&](const char* s) { return name == s; };
  if (is("layouts")) { check_layouts(); return 0; }
  if (name.rfind("prune", 0) == 0) {
    const int nc = 2, no = 5;
    std::vector<float> extr(16 * nc), ctr(3 * nc), K(9 * nc), X(3 * no), uv(2 * no), sig(no), dist(2 * no);
    std::vector<int32_t> cam = {0, 1, 1, 0, 1};
    std::vector<uint8_t> res(no);
    if (is("prune_cam")) cam[2] = 2;
    if (is("prune_negative")) cam[4] = -1;
    ba_prune_problem p{};
    p.n_cams = nc; p.n_obs = is("prune_sizes") ? -1 : no;
    p.extr = extr.data(); p.cam_center = ctr.data(); p.K = K.data(); p.obs_cam = cam.data(); p.obs_X = X.data();
    p.obs_uv = uv.data(); p.obs_inv_sigma = is("prune_null") ? nullptr : sig.data(); p.obs_dist = dist.data();
    check_prune(&p, res.data());
    return 0;
  }
  if (name.rfind("pose", 0) == 0) {
    const int n = 3;
    std::vector<int32_t> off = {0, 4, 4, 9};
    std::vector<double> cams(6 * n), pts(3 * 9), out(6 * n);
    std::vector<float> K(9 * n), uv(2 * 9);
    if (is("pose_decreasing")) off[2] = 3;
    if (is("pose_first")) off[0] = 1;
    ba_pose_batch b{};
    b.n_problems = is("pose_negative") ? -1 : n;
    b.obs_offset = off.data(); b.cams = cams.data(); b.K = K.data(); b.pts = is("pose_null") ? nullptr : pts.data();
    b.obs_uv = uv.data();
    check_pose_batch("ba_solve_pose_batch: ", &b, is("pose_out") ? nullptr : out.data());
    return 0;
  }
  if (name.rfind("tri", 0) == 0) {
    const int nc = 2, np = 3;
    std::vector<int32_t> off = {0, 2, 4, 6}, cam = {0, 1, 0, 1, 1, 0};
    std::vector<float> extr(16 * nc), ctr(3 * nc), K(9 * nc), uv(2 * 6);
    std::vector<double> init(3 * np), pts(3 * np);
    std::vector<uint8_t> st(np);
    if (is("tri_cam")) cam[1] = 5;
    if (is("tri_decreasing")) off[2] = 1;
    ba_tri_batch b{};
    b.n_cams = nc; b.n_pts = np; b.extr = extr.data(); b.cam_center = is("tri_scale") ? nullptr : ctr.data(); b.K = K.data();
    b.obs_offset = off.data(); b.obs_cam = cam.data(); b.obs_uv = uv.data();
    b.pts_init = is("tri_given_ok") ? init.data() : nullptr;
    ba_tri_options t;
    tri_defaults(t);
    if (is("tri_init")) t.init = 7;
    if (is("tri_given") || is("tri_given_ok")) t.init = BA_TRI_INIT_GIVEN;
    if (is("tri_checks")) t.checks = 64;
    if (is("tri_views")) t.min_views = -1;
    if (is("tri_solver") || is("tri_precision")) t.refine = 1;
    ba_options lm{};
    lm.linear_solver = is("tri_solver") ? BA_ITERATIVE_SCHUR : BA_DENSE_SCHUR;
    lm.precision = is("tri_precision") ? BA_MIXED_FP32 : BA_FP64;
    check_triangulate("ba_triangulate: ", &b, is("tri_defaults") ? nullptr : &t, lm, pts.data(), is("tri_out") ? nullptr : st.data());
    return 0;
  }
  if (name.rfind("window_log", 0) == 0) {
    std::printf("log_cap %zu\n", is("window_log_overflow") ? window_log_cap("ba_solve_window_batch: ", 0x7fffffff, 1 << 30)
                                                            : window_log_cap("ba_solve_window_batch: ", 50, 3));
    return 0;
  }
  if (name.rfind("hyp", 0) == 0) {
    if (is("hyp_index")) check_hypothesis_range("fn: ", "pair", 3, 3, 0, 1, 10);
    else if (is("hyp_negative")) check_hypothesis_range("fn: ", "problem", -1, 3, 0, 1, 10);
    else if (is("hyp_range")) check_hypothesis_range("fn: ", "pair", 0, 3, 5, 7, 10);
    else if (is("hyp_wrap")) check_hypothesis_range("fn: ", "pair", 0, 3, 0x7fffffff, 0x7fffffff, 10);
    else check_hypothesis_range("fn: ", "pair", 2, 3, 3, 7, 10);
    return 0;
  }
  throw std::runtime_error("unknown case " + name);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s in.bin out.bin | check NAME\n", argv[0]);
    return 2;
  }
  if (std::string(argv[1]) == "check") {
    try {
      const int rc = check_case(argv[2]);
      std::printf("ok\n");
      return rc;
    } catch (const BaError& e) {
      std::printf("error %d: %s\n", e.code, e.msg.c_str());
      return 3;
    } catch (const std::exception& e) {
      std::printf("error: %s\n", e.what());
      return 1;
    }
  }
  for (size_t align : {1, 16, 256}) {
    SectionLayout L(align);
    const size_t a = L.add(1), b = L.add(align), c = L.add(0);
    L.end_inputs();
    const size_t d = L.add(align + 1);
    L.end_outputs();
    const size_t e = L.add(700);
    std::printf("layout %zu: %zu %zu %zu %zu %zu | %zu %zu %zu\n", align, a, b, c, d, e, L.in_b, L.io_b, L.total);
  }
  offsets_message({0, 2, 2, 5}, "problem");
  offsets_message({0}, "problem");
  offsets_message({1, 2}, "problem");
  offsets_message({0, 3, 2}, "point");
  const ba_summary s1 = unpack_summary(std::vector<double>{4.0, 2.0, 7.0, 5.0, 2.0, 1.0}.data(), 0.5, false);
  const ba_summary s3 = unpack_summary(std::vector<double>{4.0, 2.0, 7.0, 5.0, 2.0, 1.0}.data(), 0.5, true);
  std::printf("summary %g %g %d %d %d %d | %g %g %g | %g %g %g\n", s1.initial_cost, s1.final_cost, s1.num_iterations,
              s1.num_successful_steps, s1.num_unsuccessful_steps, s1.termination_type, s1.total_time_s,
              s1.linearize_time_s, s1.solve_time_s, s3.total_time_s, s3.linearize_time_s, s3.solve_time_s);
  try {
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) throw std::runtime_error("cannot open the input file");
    const std::vector<int32_t> hd = get<int32_t>(f, 5);
    if (hd[0] < 0 || hd[1] < 0 || hd[2] < 0 || hd[3] < 0) throw std::runtime_error("negative size");
    const size_t n = hd[0], NC = hd[1], NP = hd[2], NO = hd[3];
    const auto cam_offset = get<int32_t>(f, n + 1), pt_offset = get<int32_t>(f, n + 1), obs_offset = get<int32_t>(f, n + 1);
    const auto cam_fixed = get<uint8_t>(f, (hd[4] & 1) ? NC : 0), pt_fixed = get<uint8_t>(f, (hd[4] & 2) ? NP : 0);
    const auto obs_cam = get<int32_t>(f, NO), obs_pt = get<int32_t>(f, NO);
    const auto obs_uv = get<float>(f, 2 * NO);
    ba_window_batch b{};
    b.n_problems = hd[0];
    b.cam_offset = cam_offset.data(); b.pt_offset = pt_offset.data(); b.obs_offset = obs_offset.data();
    b.cam_fixed = (hd[4] & 1) ? cam_fixed.data() : nullptr;
    b.pt_fixed = (hd[4] & 2) ? pt_fixed.data() : nullptr;
    b.obs_cam = obs_cam.data(); b.obs_pt = obs_pt.data(); b.obs_uv = obs_uv.data();
    const WindowPack w = pack_window_structure(b);
    std::ofstream o(argv[2], std::ios::binary);
    static_assert(sizeof(WinProb) == 12 * sizeof(int), "WinProb: 12 ints");
    put(o, w.prob); put(o, w.cam_vc); put(o, w.pt_var); put(o, w.pt_off); put(o, w.obs_cam); put(o, w.obs_slot);
    put(o, w.uv); put(o, w.cam_off); put(o, w.cam_obs);
    put(o, std::vector<int64_t>{static_cast<int64_t>(w.NV)});
    if (!o) throw std::runtime_error("cannot write the output file");
    std::printf("packed %zu problems\n", w.prob.size());
  } catch (const BaError& e) {
    std::printf("error %d: %s\n", e.code, e.msg.c_str());
    return 3;
  } catch (const std::exception& e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
  return 0;
}
