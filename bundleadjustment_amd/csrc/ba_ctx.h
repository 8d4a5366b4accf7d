// ba_ctx.h — the context behind the C ABI's ba_ctx handle and what the host
// translation units share: ba_solver.hip (structure, workspace, the LM driver,
// covariance, debug, comm, create / destroy) and ba_batch.hip (the batch entry
// points).  The error macros, the staging arena of a batch entry point with its
// whole upload / launch / download / timing protocol, the list buffers of
// ba_map_graph, and the small option helpers.  Host code only.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ba_hip.h"
#include "ba_cov_pcg.h"
#include "ba_kernels.h"

// BaError {code, msg}: host/ba_batch_pack.hpp (through ba_kernels.h)
#define HIP_OK(expr)                                                                                  \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess)                                                                             \
      throw bahip::BaError{_e == hipErrorOutOfMemory ? BA_ERR_OUT_OF_MEMORY : BA_ERR_DEVICE,          \
                           std::string(#expr) + ": " + hipGetErrorString(_e)};                        \
  } while (0)
#define NCCL_OK(expr)                                                                                 \
  do {                                                                                                \
    ncclResult_t _r = (expr);                                                                         \
    if (_r != ncclSuccess) throw bahip::BaError{BA_ERR_COMM, std::string(#expr) + ": " + ncclGetErrorString(_r)}; \
  } while (0)

// internal to the library: not among its dynamic symbols
#define BA_INTERNAL __attribute__((visibility("hidden")))

namespace bahip {

BA_INTERNAL inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <class T> BA_INTERNAL T* at(char* base, size_t off) { return reinterpret_cast<T*>(base + off); }

// The staging buffer of a batch entry point and the protocol every entry point
// follows with it.  Device memory laid out by a SectionLayout (inputs | outputs
// | scratch), grown on demand and reused across calls; the host copy of its
// inputs and outputs; the times of the last timed call.  A call runs
//   tic .. begin, put .., upload, [upload_from ..], kernels_begin, <launches>,
//   kernels_end, download, copy_out .., finish
// on the context's stream; an entry that reports no times leaves out tic,
// kernels_begin / kernels_end and finish.
//
// The host copy comes into being with the first operation that touches it, so
// an entry whose inputs all go up with upload_from and whose outputs come down
// with fetch into the caller's memory (the map graph) has none.  What goes up
// through it is never uninitialised, possibly stale, and costs no pass over
// bytes that are about to be overwritten: the copy is value-initialised where
// it grows, put writes a section and zeroes the padding behind it, and a put
// without a source zeroes the section (an absent optional input).  Whoever
// writes a section in place, or in parts, calls pad for its tail.
struct BA_INTERNAL StagingArena {
  static constexpr int kPhaseEv = 7;   // ctx->ev[kPhaseEv ..]: the phase stamps of an entry that times its phases
  char* dev = nullptr;
  size_t cap = 0;
  std::vector<char> host;
  std::vector<double> ms;   // the last timed call: host preparation (wall), kernels (device), the call (wall), extras

  StagingArena() = default;
  StagingArena(const StagingArena&) = delete;
  StagingArena& operator=(const StagingArena&) = delete;
  ~StagingArena() { (void)hipFree(dev); }

  void reserve(ba_ctx* ctx, size_t bytes, const std::string& fn);
  // the device is set and the buffer holds L.total bytes
  void begin(ba_ctx* ctx, const SectionLayout& L, const std::string& fn);
  // a section of the host copy that exists in the layout (nb > 0 only then); src null: zeros
  void put(size_t off, const void* src, size_t nb) {
    if (!nb) return;
    char* h0 = hostp();
    if (src) std::memcpy(h0 + off, src, nb); else std::memset(h0 + off, 0, nb);
    std::memset(h0 + off + nb, 0, (0 - (off + nb)) & mask);
  }
  // zeroes from `end` (the end of a section's bytes, however they were written) to the next section
  void pad(size_t end) { std::memset(hostp() + end, 0, (0 - end) & mask); }
  // enqueue: the staged prefix [0, upto); a bulk section from the caller's memory; one section to dst or the host copy
  void upload(size_t upto) { if (upto) HIP_OK(hipMemcpyAsync(dev, host.data(), upto, hipMemcpyHostToDevice, stream)); }
  void upload_from(size_t off, const void* src, size_t nb) {
    if (src && nb) HIP_OK(hipMemcpyAsync(dev + off, src, nb, hipMemcpyHostToDevice, stream));
  }
  void fetch(size_t off, size_t nb, void* dst = nullptr) {
    if (nb) HIP_OK(hipMemcpyAsync(dst ? dst : hostp() + off, dev + off, nb, hipMemcpyDeviceToHost, stream));
  }
  void download() {   // launch errors; the outputs [in_b, io_b) to the host copy; synchronises
    HIP_OK(hipGetLastError());
    fetch(in_b, io_b - in_b);
    HIP_OK(hipStreamSynchronize(stream));
  }
  void copy_out(void* dst, size_t off, size_t nb) const { if (dst && nb) std::memcpy(dst, host.data() + off, nb); }
  template <class T> T* d(size_t off) const { return reinterpret_cast<T*>(dev + off); }
  template <class T> const T* h(size_t off) const { return reinterpret_cast<const T*>(host.data() + off); }
  template <class T> T* h(size_t off) { return reinterpret_cast<T*>(hostp() + off); }

  void tic() { t0 = now_s(); t_prep = -1.0; kern = 0.0; pending = false; }
  void prepared() { if (t_prep < 0.0) t_prep = now_s() - t0; }   // the host preparation ends here (once per call)
  void kernels_begin() { prepared(); HIP_OK(hipEventRecord(ev[0], stream)); }
  void kernels_end() { HIP_OK(hipGetLastError()); HIP_OK(hipEventRecord(ev[1], stream)); pending = true; }
  double kernels_done() {   // after a synchronisation: adds the stamped pair to the call's device time, returns that
    float t = 0.0f;
    if (pending) HIP_OK(hipEventElapsedTime(&t, ev[0], ev[1]));
    pending = false;
    return kern += (double)t;
  }
  double finish(std::initializer_list<double> extra = {}) {   // stores ms, returns the call's wall time (s)
    kernels_done();
    const double wall = now_s() - t0;
    ms = {1e3 * t_prep, kern, 1e3 * wall};
    for (double e : extra) ms.push_back(e);
    return wall;
  }
  // launches that stamp the end of each of n <= 3 phases themselves: the events, and finish with the phases as extras
  hipEvent_t* phase_stamps() const { return ev + kPhaseEv; }
  double finish_phases(int n) {
    float sum = 0.0f, t[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < n; ++i) {
      HIP_OK(hipEventElapsedTime(&t[i], i ? ev[kPhaseEv + i - 1] : ev[0], ev[kPhaseEv + i]));
      sum += t[i];
    }
    kern = (double)sum;
    return finish({(double)t[0], (double)t[1], (double)t[2]});
  }

 private:
  char* hostp() { if (host.size() < io_b) host.resize(io_b); return host.data(); }   // the host copy, [0, io_b)
  hipStream_t stream = nullptr;   // the context's stream and events (begin)
  hipEvent_t* ev = nullptr;
  size_t in_b = 0, io_b = 0, mask = 0;
  double t0 = 0.0, t_prep = -1.0, kern = 0.0;   // kern: device time (ms) of this call's launch groups so far
  bool pending = false;
};

// The variable-length lists of the last ba_map_graph, on the device: the eight
// arrays of ba_graph_lists in its order, grown chunk by chunk.  len: elements
// of the neighbour, camera, point and observation lists.
struct BA_INTERNAL GraphLists {
  static constexpr int kArrays = 8;
  static constexpr size_t elem[kArrays] = {4, 4, 4, 1, 4, 4, 4, 4};
  static constexpr int kind[kArrays] = {0, 0, 1, 1, 2, 3, 3, 3};
  char* buf[kArrays] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t cap[kArrays] = {0, 0, 0, 0, 0, 0, 0, 0};   // elements
  size_t len[4] = {0, 0, 0, 0};
  bool valid = false;
  GraphLists() = default;
  GraphLists(const GraphLists&) = delete;
  GraphLists& operator=(const GraphLists&) = delete;
  ~GraphLists() { for (char* b : buf) (void)hipFree(b); }
};

}  // namespace bahip

using namespace bahip;   // (an internal header of two translation units that both say so)

struct ba_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // [0, 1]: a timed call's stamp pair, [2..5]: two r+J stamp pairs, [6]: scalar blit, [7..9]: ba_match's phase stamps
  hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int rj_slot = 0;   // the stamp pair of the next timed linearisation (bench)
  // the device linearisation state is at the candidate of the last step (a
  // speculative linearisation, enqueued behind the step's scalar record)
  bool lin_at_cand = false;

  // multi-GPU
  int nranks = 1, rank = 0;
  ncclComm_t comm = nullptr;
  // host-staged transport (ba_comm_init_host: tests of the multi-rank path
  // with several ranks on one GPU, where RCCL refuses duplicate devices)
  ba_host_allreduce_fn host_fn = nullptr;
  void* host_user = nullptr;
  std::vector<double> host_buf;

  // problem
  bool have_problem = false;
  int nc = 0, np = 0, no = 0, nvc = 0, n = 0, ld = 0;
  std::vector<int> perm;         // sorted obs -> caller obs
  std::vector<int> chol_off;     // split Cholesky task table: host step offsets (W.ctask_off)
  std::vector<int> cam_of_vc;
  std::vector<uint8_t> cam_fixed_h, pt_fixed_h;
  double huber_a = 0.0;
  DevProblem P{};
  DevWork W{};
  std::vector<void*> allocs;     // device buffers of the current problem
  double* h_scal = nullptr;      // pinned scalar record (device-mapped, coherent)
  double* d_hscal = nullptr;     // its device address
  unsigned* h_seq = nullptr;     // the record's sequence number (after the record), host / device address
  unsigned* d_hseq = nullptr;
  unsigned* d_ticket = nullptr;  // k_reduce<true>'s last-workgroup ticket (zero between launches)
  unsigned scal_seq = 0;
  // one staging arena per group of batch entry points that share inputs (a call
  // of one group never makes another reallocate); each holds the times of its
  // last timed call and frees its buffer with the context
  StagingArena pose, win, tri, pnp, tv, match, mp, mg, icp;
  GraphLists graph;                    // the lists of the last ba_map_graph (device)
  // ba_solve_window_batch: the last call's logs
  std::vector<ba_iteration> win_log;   // [n_problems][win_log_cap]
  std::vector<int> win_log_n;
  int win_log_cap = 0;

  // host copies of the sorted structure, kept for the lazily built
  // linear-solver structures (Schur pair lists / PCG duplicate pairs)
  std::vector<int> h_pt_off, h_obs_cam, h_vc;
  std::vector<uint8_t> h_pt_var;
  bool have_dense = false, have_pcg = false;
  int chol_epoch = 0;   // launches of the back substitution (hand-off flag values)
  // scalar slots whose fold a linearisation left to the step enqueued right
  // behind it (single rank: one k_reduce for both records)
  uint32_t pend_sum = 0, pend_max = 0;
  // the camera-side norms pass of such a linearisation, left to ride in the
  // step's point-elimination launch (launch_point_elim's NormsFold)
  bool norms_pend = false;
  bahip::NormsFold norms_args{};
  // a pending norms pass as its own launch (before any fold of its slots)
  void flush_norms() {
    if (!norms_pend) return;
    norms_pend = false;
    bahip::launch_cam_norms(P, W, norms_args.compute_scale != 0, norms_args.min_diag, norms_args.max_diag, stream);
  }
  const bahip::NormsFold* take_norms() {
    if (!norms_pend) return nullptr;
    norms_pend = false;
    return &norms_args;
  }
  void clear_pending() { pend_sum = pend_max = 0; norms_pend = false; }
  bool dup_diag = false;   // the dense pair list has diagonal blocks (duplicate observations)
  bool k_plain = false;    // every camera's K without skew, row 2 = (0, 0, k22) (set_problem)
  size_t pcg_ndup = 0;     // ITERATIVE_SCHUR duplicate (camera, point) pairs (ensure_pcg)
  double* tobs_buf = nullptr;   // [no][6] ITERATIVE_SCHUR per-observation products (allocated on first use)
  int max_no = 0;               // largest observation count over the ranks (collective matvec-path choice)
  // ba_covariance_iterative: the multi-column CG's scratch (allocated on first
  // use, grown on demand, freed with the problem) and its capacity in columns
  bahip::McgBufs mcg{};
  int mcg_cols = 0;

  // solver state
  std::vector<ba_iteration> log;
  std::vector<double> bench_ms;   // host wall time of each iteration of the last ba_bench_iterations
  std::vector<double> cov_ms;     // device time of the phases of the last ba_covariance
  bool scale_valid = false;
  double t_lin = 0.0, t_solve = 0.0;

  template <typename T>
  T* dalloc(size_t count) {
    if (count == 0) count = 1;
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, count * sizeof(T)));
    allocs.push_back(p);
    return static_cast<T*>(p);
  }
  void dfree(void* p) {
    if (!p) return;
    auto it = std::find(allocs.begin(), allocs.end(), p);
    if (it != allocs.end()) allocs.erase(it);
    if (stream) (void)hipStreamSynchronize(stream);
    (void)hipFree(p);
  }
  template <typename T>
  T* upload(const std::vector<T>& v) {
    T* d = dalloc<T>(v.size());
    if (!v.empty()) HIP_OK(hipMemcpyAsync(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return d;
  }
  void free_problem() {
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    have_problem = have_dense = have_pcg = false;
    tobs_buf = nullptr;
    mcg = bahip::McgBufs{};
    mcg_cols = 0;
    scale_valid = false;
    log.clear();
  }

  // collectives on the data path: with more than one rank, or forced on a
  // one-rank communicator (BA_FORCE_COLLECTIVES=1: tests of the exchange path
  // on a single GPU, where the all-reduce is the identity)
  bool force_coll = false;
  bool has_comm() const { return comm || host_fn; }
  bool coll() const { return has_comm() && (nranks > 1 || force_coll); }
  void allreduce(double* d, size_t count, ncclRedOp_t op = ncclSum) {
    if (!has_comm() || count == 0) return;   // a 1-rank communicator still runs the collectives (tests)
    if (host_fn) {   // stage through the host and the caller's transport
      host_buf.resize(count);
      HIP_OK(hipMemcpyAsync(host_buf.data(), d, sizeof(double) * count, hipMemcpyDeviceToHost, stream));
      HIP_OK(hipStreamSynchronize(stream));
      if (host_fn(host_user, host_buf.data(), (int64_t)count, op == ncclMax ? 1 : 0) != 0)
        throw BaError{BA_ERR_COMM, "host all-reduce callback failed"};
      HIP_OK(hipMemcpyAsync(d, host_buf.data(), sizeof(double) * count, hipMemcpyHostToDevice, stream));
      // host_buf is pageable and reused by the next call: wait for the copy
      // (test transport, latency irrelevant)
      HIP_OK(hipStreamSynchronize(stream));
      return;
    }
    NCCL_OK(ncclAllReduce(d, d, count, ncclDouble, op, comm, stream));
  }
  // host values (set_problem structure, bench timing); one device scratch
  // buffer, grown on demand and kept for the context's lifetime
  double* hv_scratch = nullptr;
  size_t hv_cap = 0;
  void allreduce_host_values(double* v, size_t count, int op) {
    if (!has_comm() || count == 0) return;
    if (count > hv_cap) {
      if (hv_scratch) { (void)hipStreamSynchronize(stream); (void)hipFree(hv_scratch); hv_scratch = nullptr; hv_cap = 0; }
      HIP_OK(hipMalloc(&hv_scratch, sizeof(double) * count));
      hv_cap = count;
    }
    HIP_OK(hipMemcpyAsync(hv_scratch, v, sizeof(double) * count, hipMemcpyHostToDevice, stream));
    allreduce(hv_scratch, count, op == 1 ? ncclMax : ncclSum);
    HIP_OK(hipMemcpyAsync(v, hv_scratch, sizeof(double) * count, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
  }
  // The scalar record to the host: a one-workgroup kernel stores it into the
  // pinned, device-mapped record and then a sequence number (system-scope
  // release), and the host spins on that number, instead of a D2H blit and
  // a stream synchronisation (whose wake-up left ~20 us of idle device
  // between an LM step and the next linearisation).  A device error or a
  // missing number (bounded wait) falls back to the synchronisation, which
  // reports it.  BA_SCAL_SPIN=0: the blit + synchronisation (A/B).
  // publish_scalars() enqueues the record's transfer, wait_scalars() waits
  // for it (work enqueued in between keeps the device busy meanwhile)
  void read_scalars() {
    publish_scalars();
    wait_scalars();
  }
  bool scal_spin() const { return spin && d_hscal; }
  // per-call switches (read at every ba_solve / ba_bench_iterations entry, so
  // tests can A/B them in one process): BA_SPEC_LIN=0 turns the speculative
  // linearisation off, BA_SCAL_SPIN=0 the spin-published scalar record
  bool spec_lin = true, spin = true;
  void read_env() {
    const char* e = std::getenv("BA_SPEC_LIN");
    spec_lin = !(e && e[0] == '0');
    e = std::getenv("BA_SCAL_SPIN");
    spin = !(e && e[0] == '0');
  }
  void publish_scalars() {
    const size_t cnt = kNumSlots + kPcgState;
    flush_norms();
    if (!scal_spin()) {
      if (pend_sum | pend_max) bahip::launch_reduce(W, pend_sum, pend_max, stream);
      pend_sum = pend_max = 0;
      HIP_OK(hipMemcpyAsync(h_scal, W.scal, sizeof(double) * cnt, hipMemcpyDeviceToHost, stream));
      HIP_OK(hipEventRecord(ev[6], stream));
      return;
    }
    // scalars still to be folded (pend_*: the step's and the deferred
    // linearisation's, single rank): one launch folds and publishes them
    if ((pend_sum | pend_max) && d_ticket) {
      bahip::launch_reduce_publish(W, pend_sum, pend_max, d_hscal, (int)cnt, d_hseq, ++scal_seq, d_ticket, stream);
      pend_sum = pend_max = 0;
    } else {
      if (pend_sum | pend_max) bahip::launch_reduce(W, pend_sum, pend_max, stream);
      pend_sum = pend_max = 0;
      bahip::launch_publish_scalars(W.scal, d_hscal, (int)cnt, d_hseq, ++scal_seq, stream);
    }
    HIP_OK(hipGetLastError());
  }
  void wait_scalars() {
    if (!scal_spin()) {
      HIP_OK(hipEventSynchronize(ev[6]));
      return;
    }
    const unsigned seq = scal_seq;
    const double t0 = now_s();
    for (unsigned it = 1;; ++it) {
      if (__atomic_load_n(h_seq, __ATOMIC_ACQUIRE) == seq) return;
      if ((it & 1023u) == 0 && now_s() - t0 > 2.0) break;
    }
    HIP_OK(hipStreamSynchronize(stream));   // (raises a device error)
    if (__atomic_load_n(h_seq, __ATOMIC_ACQUIRE) != seq)
      throw BaError{BA_ERR_DEVICE, "scalar record: sequence number not received"};
  }
};

namespace bahip {

// Room for `bytes`.  Growing waits for the stream before it frees the old
// buffer; a failed allocation leaves the arena empty and no sticky error, so
// the context stays usable.
inline void StagingArena::reserve(ba_ctx* ctx, size_t bytes, const std::string& fn) {
  if (bytes <= cap) return;
  if (dev) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(dev); }
  dev = nullptr; cap = 0;
  const hipError_t e = hipMalloc(&dev, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    dev = nullptr;
    throw BaError{e == hipErrorOutOfMemory ? BA_ERR_OUT_OF_MEMORY : BA_ERR_DEVICE,
                  fn + "scratch of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e)};
  }
  cap = bytes;
}

inline void StagingArena::begin(ba_ctx* ctx, const SectionLayout& L, const std::string& fn) {
  HIP_OK(hipSetDevice(ctx->device));
  reserve(ctx, L.total, fn);
  stream = ctx->stream; ev = ctx->ev; in_b = L.in_b; io_b = L.io_b; mask = L.mask;
}

BA_INTERNAL inline ba_options options_or_default(const ba_options* opt) {
  ba_options o;
  if (opt) o = *opt; else ba_default_options(&o);
  return o;
}
BA_INTERNAL inline PoseOpts pose_opts(const ba_options& o) {
  return PoseOpts{o.max_num_iterations, o.max_num_consecutive_invalid_steps, o.jacobi_scaling,
                  o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance, o.initial_trust_region_radius,
                  o.max_trust_region_radius, o.min_trust_region_radius, o.min_relative_decrease, o.min_lm_diagonal,
                  o.max_lm_diagonal};
}
// the *_times getters: up to n values into ms, returns how many there are
BA_INTERNAL inline int copy_times(const std::vector<double>& t, double* ms, int n) {
  const int m = (int)t.size();
  for (int i = 0; i < std::min(n, m) && ms; ++i) ms[i] = t[i];
  return m;
}

// an entry point's body: the error into the context, the code returned
template <typename F>
BA_INTERNAL int guarded(ba_ctx* ctx, F&& f) {
  try {
    f();
    return BA_OK;
  } catch (const BaError& e) {
    if (ctx) ctx->err = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    if (ctx) ctx->err = e.what();
    return BA_ERR_DEVICE;
  } catch (...) {
    if (ctx) ctx->err = "unknown error";
    return BA_ERR_DEVICE;
  }
}

}  // namespace bahip

