// gicp.hip -- generalized (plane-to-plane) ICP refinement (Segal, Haehnel & Thrun; pcl::GeneralizedIterativeClosestPoint's
// plane-to-plane covariances, fast_gicp's Gauss-Newton step) behind the registration's exact 1-NN search.  Host side of
// gicp_kernels.hpp; tests/gicp_ref.py is the contract.  The C entry points are in reg.hip (they own the handle's layout
// and the 1-NN passes) and call run() here.
//
// Every pair is weighted by M = (C_B + R C_A R^T)^-1, frozen at the pass's linearisation point: Gauss-Newton, not PCL's
// BFGS inner loop.  The loop of passes is gn6.hpp's, shared with the point-to-plane refinement.
#include "gicp.hpp"
#include "gicp_kernels.hpp"
#include "gn6.hpp"

using namespace gloc;
using namespace gloc::gicp;

namespace gloc {
namespace gicp {

int check_params(const gloc_gicp_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->max_iters >= 1 && p->max_iters <= 10000, GLOC_ERR_INVALID, "max_iters = %u outside [1, 10000]", p->max_iters);
  GLOC_REQUIRE(p->normal_k >= 3 && p->normal_k <= 16, GLOC_ERR_INVALID, "normal_k = %u outside [3, 16]", p->normal_k);
  GLOC_REQUIRE(p->plane_eps > 0.f && p->plane_eps <= 1.f, GLOC_ERR_INVALID, "plane_eps = %g outside (0, 1]", (double)p->plane_eps);
  return GLOC_OK;
}

int run(const p2l::Ctx& x, const Target* tgts, const gn6::Call& call, const gloc_gicp_params* prm) {
  const gn6::Loop lp{prm->max_iters, prm->max_corr_dist, prm->trans_eps, prm->rot_eps, "gicp_accum", "gicp_solve"};
  const double a = 1.0 - (double)prm->plane_eps;
  auto accum = [&](const Target* d_tgts, const gn6::Source* d_srcs, const State* states, float gate2, bool skip_stopped, double* partials,
                   uint32_t n_blk, const gn6::Scale2& sc) {
    gn6::for_kind(call.kind(), [&](auto kind) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(gicp_accum_kernel<decltype(kind)::value>), dim3(n_blk, x.n_jobs), dim3(ACC_THREADS), 0, x.stream,
                         d_srcs, d_tgts, x.pose_f32, x.pose_stride, states, x.corr, x.d2, x.ld, gate2, a, skip_stopped,
                         partials, sc);
    });
  };
  return gn6::run(x, lp, tgts, call, accum);
}

}  // namespace gicp
}  // namespace gloc

extern "C" {

void gloc_gicp_default_params(gloc_gicp_params* p) {
  if (!p) return;
  p->max_iters = 30;  // registration/global_registration.cpp:242
  p->max_corr_dist = 0.f;
  p->trans_eps = 0.f;
  p->rot_eps = 0.f;
  p->normal_k = 10;  // registration/ground_estimator.cpp:79
  p->plane_eps = 1e-3f;
}

}  // extern "C"
