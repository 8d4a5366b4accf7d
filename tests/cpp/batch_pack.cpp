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

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
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
