// gn6.hpp -- the host side the Gauss-Newton refinements share (p2l.hip, gicp.hip, vgicp.hip): the handle's workspace and the
// loop of passes.  A pass is three enqueues: the registration's exact 1-NN search (none for the voxelized refinement,
// whose Ctx::nn_pass is null), the refinement's own accumulate kernel, the solve kernel of gn6_kernels.hpp.  What is asked
// for -- the guesses, a batch or ONE evaluation of the system, the outputs, the robust block -- arrives as the gn6::Call
// (p2l.hpp) the C entry filled.
//
// Synchronisation between passes: none.  Whether a job has stopped is a flag on the device that the accumulate and solve
// kernels of later passes read.  With both eps off a job can only stop early by being degenerate, so all max_iters passes
// go in back to back; with eps set the host looks at the count of stopped jobs every LOOK_EVERY passes -- one 4-byte copy
// and an event -- to cut the tail once every job has stopped.
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>

#include "gn6_kernels.hpp"
#include "p2l.hpp"

namespace gloc {
namespace p2l {

struct Ws {  // (one per handle, whichever refinement runs: the calls are synchronous)
  DevBuf tgts, srcs, states, partials, done, exp, c2tab;
  uint32_t* h_done = nullptr;  // pinned
  hipEvent_t ev = nullptr;
  ~Ws() {
    if (h_done) (void)hipHostFree(h_done);
    if (ev) (void)hipEventDestroy(ev);
  }
};

}  // namespace p2l

namespace gn6 {

constexpr uint32_t LOOK_EVERY = 4;

// f(std::integral_constant<int, KIND>) for the robust kind of a call: the accumulate kernels are templates on it
template <class F>
void for_kind(uint32_t kind, F&& f) {
  switch (kind) {
    case GLOC_ROBUST_HUBER: f(std::integral_constant<int, GLOC_ROBUST_HUBER>()); break;
    case GLOC_ROBUST_CAUCHY: f(std::integral_constant<int, GLOC_ROBUST_CAUCHY>()); break;
    case GLOC_ROBUST_TUKEY: f(std::integral_constant<int, GLOC_ROBUST_TUKEY>()); break;
    case GLOC_ROBUST_GEMAN_MCCLURE: f(std::integral_constant<int, GLOC_ROBUST_GEMAN_MCCLURE>()); break;
    default: f(std::integral_constant<int, GLOC_ROBUST_NONE>());
  }
}

struct Loop {  // what the refinements' parameter blocks have in common
  uint32_t max_iters;
  float max_corr_dist, trans_eps, rot_eps;
  const char *accum_name, *solve_name;  // in the handle's profile
};

// Refines every job of `call` from its init_T, or with call.system evaluates every job ONCE at it (the single-pair entries
// have one).  `tgts` [x.n_jobs]: the
// jobs' targets as the accumulate kernel takes them, copied to the device beside the table of the jobs' sources
// (gn6::Source, made here from x.srcs: every job's work-group count and its first row of the partials); accum(targets and
// sources on the device, states, gate^2, skip_stopped, partials, the grid's width -- the largest work-group count --, the
// pass's Scale2) enqueues that kernel.  Returns after the results have been copied out.
//
// call.robust (robust.hpp): with a kind other than NONE accum is also handed the pass's scale -- the table of c(k)^2 made
// here with the host helper's own function, indexed by each job's update count, during the loop; scale^2 for the
// evaluation after it; c(call.pass)^2 for the system form -- and the solve kernel the first update index at which the
// stop test counts.
template <class Target, class Accum>
int run(const p2l::Ctx& x, const Loop& lp, const Target* tgts, const Call& call, Accum&& accum) {
  const float* init_T = call.init_T;
  const gloc_robust_params* rb = call.robust;
  if (!*x.ws) {
    *x.ws = new (std::nothrow) p2l::Ws;
    GLOC_REQUIRE(*x.ws, GLOC_ERR_NOMEM, "host allocation failed");
  }
  p2l::Ws& w = **x.ws;
  const hipStream_t q = x.stream;
  const uint32_t n = x.n_jobs;
  const bool weighted = call.kind() != GLOC_ROBUST_NONE;
  // a job's work-groups and rows depend on its own source alone: the partition a call on the job alone makes
  std::vector<Source> hsrc(n);
  uint64_t n_rows = 0;
  uint32_t n_blk = 1;  // the grid's width
  for (uint32_t c = 0; c < n; ++c) {
    const p2l::SourceView& sv = x.srcs[c];
    const uint32_t nb = (uint32_t)(((uint64_t)sv.n + ACC_THREADS - 1) / ACC_THREADS);
    hsrc[c] = Source{sv.pts, sv.nrm, sv.n, nb, n_rows};
    n_rows += nb;
    n_blk = std::max(n_blk, nb);
  }
  std::vector<State> hs(n);
  static const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  for (uint32_t c = 0; c < n; ++c) {
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
  GLOC_TRY(w.srcs.ensure(sizeof(Source) * n, q));
  GLOC_TRY(w.partials.ensure(sizeof(double) * NSLOT * (size_t)std::max<uint64_t>(n_rows, 1), q));
  GLOC_TRY(w.done.ensure(16, q));
  GLOC_TRY(w.exp.ensure(sizeof(double) * NSUM * n, q));
  if (!w.h_done) GLOC_HIP(hipHostMalloc(reinterpret_cast<void**>(&w.h_done), 16, hipHostMallocDefault));
  if (!w.ev) GLOC_HIP(hipEventCreateWithFlags(&w.ev, hipEventDisableTiming));
  GLOC_HIP(hipMemcpyAsync(w.tgts.p, tgts, sizeof(Target) * n, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.srcs.p, hsrc.data(), sizeof(Source) * n, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemcpyAsync(w.states.p, hs.data(), sizeof(State) * n, hipMemcpyHostToDevice, q));
  GLOC_HIP(hipMemsetAsync(w.done.p, 0, 16, q));
  // the scales: c(k)^2 for k = 0 .. the last update index a job can have, cut where the schedule has settled
  std::vector<double> c2;
  uint32_t stop_from = 0;
  Scale2 loop_sc{nullptr, 0, 0.0}, end_sc{nullptr, 0, 0.0};
  if (weighted) {
    if (call.system) {
      const double c = robust::scale_at(rb, call.pass);
      end_sc.fixed = c * c;
    } else {
      stop_from = 0xFFFFFFFFu;  // (a schedule that has not settled by the last update: no update's stop test counts)
      double c = robust::scale_first(rb);
      for (uint32_t k = 0; k < lp.max_iters; ++k, c = robust::scale_next(rb, c)) {
        c2.push_back(c * c);
        if (c == (double)rb->scale) {
          stop_from = k;
          break;
        }
      }
      const uint32_t n_tab = (uint32_t)c2.size();
      GLOC_TRY(w.c2tab.ensure(sizeof(double) * n_tab, q));
      GLOC_HIP(hipMemcpyAsync(w.c2tab.p, c2.data(), sizeof(double) * n_tab, hipMemcpyHostToDevice, q));
      loop_sc = Scale2{w.c2tab.template as<double>(), n_tab, 0.0};
      end_sc.fixed = (double)rb->scale * (double)rb->scale;
    }
  }
  GLOC_HIP(hipStreamSynchronize(q));  // (tgts, hsrc and hs are host memory)
  const float gate2 = lp.max_corr_dist > 0.f ? lp.max_corr_dist * lp.max_corr_dist : 0.f;
  bool warm = false;
  // search, accumulate, solve at the current poses; mode 1: evaluation only
  auto pass = [&](int mode, double* exp) -> int {
    if (x.nn_pass) GLOC_TRY(x.nn_pass(x.self, warm));  // (null: the accumulate kernel finds its own pairs -- vgicp.hip)
    warm = true;
    {
      ProfScope ps(*x.prof, lp.accum_name, q);
      accum(w.tgts.template as<Target>(), w.srcs.template as<Source>(), w.states.template as<State>(), gate2, mode == 0,
            w.partials.template as<double>(), n_blk, mode == 0 ? loop_sc : end_sc);
    }
    {
      ProfScope ps(*x.prof, lp.solve_name, q);
      hipLaunchKernelGGL(solve_kernel, dim3(n), dim3(64), 0, q, w.partials.template as<double>(), w.srcs.template as<Source>(),
                         stop_from, w.states.template as<State>(), x.pose_f32, x.pose_stride, (double)lp.trans_eps, (double)lp.rot_eps, mode,
                         w.done.template as<uint32_t>(), exp);
    }
    GLOC_HIP(hipGetLastError());
    return GLOC_OK;
  };
  if (call.system) {
    // (a single-pair entry: n = 1; a list: every job evaluated by the one pass, the sums of all of them in one copy)
    GLOC_TRY(pass(1, w.exp.template as<double>()));
    std::vector<double> sums((size_t)NSUM * n);
    GLOC_HIP(hipMemcpyAsync(sums.data(), w.exp.p, sizeof(double) * NSUM * n, hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipMemcpyAsync(hs.data(), w.states.p, sizeof(State) * n, hipMemcpyDeviceToHost, q));
    GLOC_HIP(hipStreamSynchronize(q));
    for (uint32_t c = 0; c < n; ++c) {
      const double* s = sums.data() + (size_t)NSUM * c;
      if (call.out_H36) {
        double* H = call.out_H36 + 36 * (size_t)c;
        int e = 0;
        for (int a = 0; a < 6; ++a)
          for (int b = a; b < 6; ++b, ++e) H[6 * a + b] = H[6 * b + a] = s[e];
      }
      if (call.out_g6) std::copy(s + 21, s + 27, call.out_g6 + 6 * (size_t)c);
      if (call.out_sum) call.out_sum[c] = s[27];
      if (call.out_count) call.out_count[c] = (uint64_t)s[28];
      if (call.out_wsum) call.out_wsum[c] = weighted ? hs[c].wsum : s[28];  // (kind NONE: every pair's weight is 1)
    }
    return GLOC_OK;
  }
  const bool can_converge = lp.trans_eps > 0.f && lp.rot_eps > 0.f;
  for (uint32_t it = 0; it < lp.max_iters; ++it) {
    GLOC_TRY(pass(0, nullptr));
    if (can_converge && (it + 1) % LOOK_EVERY == 0 && it + 1 < lp.max_iters) {
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
    if (call.out_T) {
      float* T = call.out_T + 16 * (size_t)c;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)s.Td[3 * i + j];
        T[4 * i + 3] = (float)s.Td[9 + i];
      }
      T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    }
    if (call.out_rmse) call.out_rmse[c] = (float)s.rmse;
    if (call.out_iters) call.out_iters[c] = s.iters;
    if (call.out_status) call.out_status[c] = s.status;
    if (call.out_weight) call.out_weight[c] = s.count == 0 ? 0.f : weighted ? (float)(s.wsum / (double)s.count) : 1.f;
  }
  return GLOC_OK;
}

}  // namespace gn6
}  // namespace gloc
