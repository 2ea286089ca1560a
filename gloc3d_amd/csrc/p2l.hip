// p2l.hip -- point-to-plane ICP refinement (Chen & Medioni's linearised step, as PCL's IterativeClosestPointWithNormals
// and Open3D's TransformationEstimationPointToPlane take it) behind the registration's exact 1-NN search.  Host side of
// p2l_kernels.hpp; tests/p2l_ref.py is the contract.  The C entry points are in reg.hip (they own the handle's layout
// and the 1-NN passes) and call run() here.
//
// Synchronisation between passes: none.  A pass is three enqueues (search, accumulate, solve); whether a job has stopped
// is a flag on the device that the accumulate and solve kernels of later passes read.  With both eps off a job can only
// stop early by being degenerate, so all max_iters passes go in back to back; with eps set the host looks at the count of
// stopped jobs every LOOK_EVERY passes -- one 4-byte copy and an event -- to cut the tail once every job has stopped.
#include <algorithm>
#include <vector>

#include "p2l.hpp"
#include "p2l_kernels.hpp"

using namespace gloc;
using namespace gloc::p2l;

namespace gloc {
namespace p2l {

struct Ws {
  DevBuf tgts, states, partials, done, exp;
  uint32_t* h_done = nullptr;  // pinned
  hipEvent_t ev = nullptr;
  ~Ws() {
    if (h_done) (void)hipHostFree(h_done);
    if (ev) (void)hipEventDestroy(ev);
  }
};

void ws_free(Ws* w) { delete w; }

namespace {
constexpr uint32_t LOOK_EVERY = 4;
}

int check_params(const gloc_p2l_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->max_iters >= 1 && p->max_iters <= 10000, GLOC_ERR_INVALID, "max_iters = %u outside [1, 10000]", p->max_iters);
  GLOC_REQUIRE(p->normal_k >= 3 && p->normal_k <= 16, GLOC_ERR_INVALID, "normal_k = %u outside [3, 16]", p->normal_k);
  return GLOC_OK;
}

int run(const Ctx& x, const TargetView* tgts, const float* init_T, const gloc_p2l_params* prm, float* out_T, float* out_rmse,
        uint32_t* out_iters, int* out_status, double* out_H36, double* out_g6, double* out_sum_r2, uint64_t* out_count) {
  if (!*x.ws) {
    *x.ws = new (std::nothrow) Ws;
    GLOC_REQUIRE(*x.ws, GLOC_ERR_NOMEM, "host allocation failed");
  }
  Ws& w = **x.ws;
  const hipStream_t q = x.stream;
  const uint32_t n = x.n_jobs;
  const bool system = out_H36 || out_g6 || out_sum_r2 || out_count;
  const uint32_t n_blk = std::max<uint32_t>(1, (x.n_src + ACC_THREADS - 1) / ACC_THREADS);
  std::vector<Target> ht(n);
  std::vector<State> hs(n);
  static const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (uint32_t c = 0; c < n; ++c) {
    ht[c] = Target{tgts[c].pts, tgts[c].nrm, tgts[c].n, 0u};
    State& s = hs[c];
    memset(&s, 0, sizeof(s));
    const float* T = init_T ? init_T + 16 * (size_t)c : I16;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) s.Td[3 * i + j] = (double)T[4 * i + j];
      s.Td[9 + i] = (double)T[4 * i + 3];
    }
  }
  GLOC_TRY(w.tgts.ensure(sizeof(Target) * n, q));
  GLOC_TRY(w.states.ensure(sizeof(State) * n, q));
  GLOC_TRY(w.partials.ensure(sizeof(double) * NSLOT * (size_t)n_blk * n, q));
  GLOC_TRY(w.done.ensure(16, q));
  GLOC_TRY(w.exp.ensure(sizeof(double) * NSUM * n, q));
  if (!w.h_done) GLOC_HIP(hipHostMalloc(reinterpret_cast<void**>(&w.h_done), 16, hipHostMallocDefault));
  if (!w.ev) GLOC_HIP(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
  GLOC_HIP(hipMemcpyAsync(w.tgts.p, ht.data(), sizeof(Target) * n, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.states.p, hs.data(), sizeof(State) * n, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemsetAsync(w.done.p, 0, 16, q));
  GLOC_HIP(hipStreamSynchronize(q));  // (ht and hs are locals)
  const float gate2 = prm->max_corr_dist > 0.f ? prm->max_corr_dist * prm->max_corr_dist : 0.f;
  bool warm = false;
  // search, accumulate, solve at the current poses; mode 1: evaluation only
  auto pass = [&](int mode, double* exp) -> int {
    GLOC_TRY(x.nn_pass(x.self, warm));
    warm = true;
    {
      ProfScope ps(*x.prof, "p2l_accum", q);
      hipLaunchKernelGGL(p2l_accum_kernel, dim3(n_blk, n), dim3(ACC_THREADS), 0, q, x.src_pts, x.n_src, w.tgts.as<Target>(),
                         x.pose_f32, x.pose_stride, w.states.as<State>(), x.corr, x.d2, x.ld, gate2, mode == 0,
                         w.partials.as<double>());
    }
    {
      ProfScope ps(*x.prof, "p2l_solve", q);
      hipLaunchKernelGGL(p2l_solve_kernel, dim3(n), dim3(64), 0, q, w.partials.as<double>(), n_blk, w.states.as<State>(),
                         x.pose_f32, x.pose_stride, (double)prm->trans_eps, (double)prm->rot_eps, mode, w.done.as<uint32_t>(), exp);
    }
    GLOC_HIP(hipGetLastError());
    return GLOC_OK;
  };
  if (system) {
    GLOC_TRY(pass(1, w.exp.as<double>()));
    double s[NSUM];
    GLOC_HIP(hipMemcpyAsync(s, w.exp.p, sizeof(double) * NSUM, hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipStreamSynchronize(q));
    if (out_H36) {
      int e = 0;
      for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b, ++e) out_H36[6 * a + b] = out_H36[6 * b + a] = s[e];
    }
    if (out_g6) std::copy(s + 21, s + 27, out_g6);
    if (out_sum_r2) *out_sum_r2 = s[27];
    if (out_count) *out_count = (uint64_t)s[28];
    return GLOC_OK;
  }
  const bool can_converge = prm->trans_eps > 0.f && prm->rot_eps > 0.f;
  for (uint32_t it = 0; it < prm->max_iters; ++it) {
    GLOC_TRY(pass(0, nullptr));
    if (can_converge && (it + 1) % LOOK_EVERY == 0 && it + 1 < prm->max_iters) {
      GLOC_HIP(hipMemcpyAsync(w.h_done, w.done.p, 4, hipMemcpyDeviceToHost, q));
      GLOC_HIP(hipEventRecord(w.ev, q));
      GLOC_HIP(hipEventSynchronize(w.ev));
      if (*w.h_done >= n) break;
    }
  }
  GLOC_TRY(pass(1, nullptr));  // the residual at the final pose
  GLOC_HIP(hipMemcpyAsync(hs.data(), w.states.p, sizeof(State) * n, hipMemcpyDeviceToHost, q));
  GLOC_HIP(hipStreamSynchronize(q));
  for (uint32_t c = 0; c < n; ++c) {
    const State& s = hs[c];
    if (out_T) {
      float* T = out_T + 16 * (size_t)c;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)s.Td[3 * i + j];
        T[4 * i + 3] = (float)s.Td[9 + i];
      }
      T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    }
    if (out_rmse) out_rmse[c] = (float)s.rmse;
    if (out_iters) out_iters[c] = s.iters;
    if (out_status) out_status[c] = s.status;
  }
  return GLOC_OK;
}

}  // namespace p2l
}  // namespace gloc

extern "C" {

void gloc_p2l_default_params(gloc_p2l_params* p) {
  if (!p) return;
  p->max_iters = 30;  // registration/global_registration.cpp:242
  p->max_corr_dist = 0.f;
  p->trans_eps = 0.f;
  p->rot_eps = 0.f;
  p->normal_k = 10;   // registration/ground_estimator.cpp:79
  p->reserved_ = 0;
}

}  // extern "C"
