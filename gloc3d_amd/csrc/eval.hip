// eval.hip -- the point-to-point evaluation of registered pairs: fitness, inlier RMSE, correspondence count and the 6 x 6
// information matrix of a list of (source, target, pose) rows (gloc_reg_evaluate_pairs).  Host side of eval_kernels.hpp;
// tests/eval_ref.py is the contract.  The C entry is in reg.hip (it owns the handle's layout and the 1-NN pass) and calls
// run() here.
//
// Nothing is reduced here: the evaluation is the system form of gn6.hpp's loop of passes over a pair list -- one cold
// 1-NN pass, the accumulate kernel, the shared solve kernel in evaluation mode, one copy of every job's 29 sums -- and the
// figures are formed from those sums on the host.
#include <cmath>
#include <vector>

#include "eval.hpp"
#include "eval_kernels.hpp"
#include "gn6.hpp"

namespace gloc {
namespace eval {

int check_params(const gloc_eval_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->max_corr_dist > 0.f && p->max_corr_dist <= 3.4028235e38f, GLOC_ERR_INVALID,
               "max_corr_dist = %g must be > 0 and finite", (double)p->max_corr_dist);
  return GLOC_OK;
}

int run(const p2l::Ctx& x, const gn6::Target* tgts, const float* T, const gloc_eval_params* prm, const Out& out) {
  const size_t n = x.n_jobs;
  std::vector<double> H(36 * n), g(6 * n), sum(n);
  std::vector<uint64_t> cnt(n);
  gn6::Call call;
  call.pairs = true;
  call.n = n;
  call.init_T = T;
  call.system = true;
  call.out_H36 = H.data();
  call.out_g6 = g.data();
  call.out_sum = sum.data();
  call.out_count = cnt.data();
  const gn6::Loop lp{1, prm->max_corr_dist, 0.f, 0.f, "eval_accum", "eval_solve"};
  auto accum = [&](const gn6::Target* d_tgts, const gn6::Source* d_srcs, const gn6::State*, float gate2, bool, double* partials,
                   uint32_t n_blk, const gn6::Scale2&) {
    hipLaunchKernelGGL(eval_accum_kernel, dim3(n_blk, x.n_jobs), dim3(gn6::ACC_THREADS), 0, x.stream, d_srcs, d_tgts, x.pose_f32,
                       x.pose_stride, x.corr, x.d2, x.ld, gate2, partials);
  };
  GLOC_TRY(gn6::run(x, lp, tgts, call, accum));
  for (size_t c = 0; c < n; ++c) {
    const uint64_t k = cnt[c];
    // V5 (a row without a target has no source slot and no pair: x.srcs[c].n is 0 there and never divides)
    if (out.fitness) out.fitness[c] = k ? (float)((double)k / (double)x.srcs[c].n) : 0.f;
    if (out.rmse) out.rmse[c] = k ? (float)std::sqrt(sum[c] / (double)k) : 0.f;
    if (out.count) out.count[c] = (uint32_t)k;
    if (out.info36) std::copy(H.begin() + 36 * c, H.begin() + 36 * (c + 1), out.info36 + 36 * c);
    if (out.g6) std::copy(g.begin() + 6 * c, g.begin() + 6 * (c + 1), out.g6 + 6 * c);
  }
  return GLOC_OK;
}

}  // namespace eval
}  // namespace gloc

extern "C" {

void gloc_eval_default_params(gloc_eval_params* p) {
  if (!p) return;
  p->max_corr_dist = 0.6f;  // 3 * 0.2 m: registration/loop_detector.cpp:257, the library's inlier_thresh
  p->reserved_ = 0;
}

}  // extern "C"
