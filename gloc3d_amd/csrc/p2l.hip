// p2l.hip -- point-to-plane ICP refinement (Chen & Medioni's linearised step, as PCL's IterativeClosestPointWithNormals
// and Open3D's TransformationEstimationPointToPlane take it) behind the registration's exact 1-NN search.  Host side of
// p2l_kernels.hpp; tests/p2l_ref.py is the contract.  The C entry points are in reg.hip (they own the handle's layout
// and the 1-NN passes) and call run() here.
//
// The loop of passes is gn6.hpp's, shared with the generalized ICP.
#include "gn6.hpp"
#include "p2l.hpp"
#include "p2l_kernels.hpp"
#include "robust.hpp"

using namespace gloc;
using namespace gloc::p2l;

namespace gloc {
namespace p2l {

void ws_free(Ws* w) { delete w; }

int check_params(const gloc_p2l_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->max_iters >= 1 && p->max_iters <= 10000, GLOC_ERR_INVALID, "max_iters = %u outside [1, 10000]", p->max_iters);
  GLOC_REQUIRE(p->normal_k >= 3 && p->normal_k <= 16, GLOC_ERR_INVALID, "normal_k = %u outside [3, 16]", p->normal_k);
  return GLOC_OK;
}

int run(const Ctx& x, const Target* tgts, const gn6::Call& call, const gloc_p2l_params* prm) {
  const gn6::Loop lp{prm->max_iters, prm->max_corr_dist, prm->trans_eps, prm->rot_eps, "p2l_accum", "p2l_solve"};
  auto accum = [&](const Target* d_tgts, const gn6::Source* d_srcs, const State* states, float gate2, bool skip_stopped, double* partials,
                   uint32_t n_blk, const gn6::Scale2& sc) {
    gn6::for_kind(call.kind(), [&](auto kind) {
      hipLaunchKernelGGL(HIP_KERNEL_NAME(p2l_accum_kernel<decltype(kind)::value>), dim3(n_blk, x.n_jobs), dim3(ACC_THREADS), 0, x.stream,
                         d_srcs, d_tgts, x.pose_f32, x.pose_stride, states, x.corr, x.d2, x.ld, gate2, skip_stopped, partials, sc);
    });
  };
  return gn6::run(x, lp, tgts, call, accum);
}

}  // namespace p2l

namespace robust {

int check_params(const gloc_robust_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "robust params is null");
  GLOC_REQUIRE(p->kind <= GLOC_ROBUST_GEMAN_MCCLURE, GLOC_ERR_INVALID, "robust kind = %u is not one of 0 .. 4", p->kind);
  if (p->kind == GLOC_ROBUST_NONE) return GLOC_OK;
  GLOC_REQUIRE(p->scale > 0.f && p->scale <= 3.4028235e38f, GLOC_ERR_INVALID, "robust scale = %g must be > 0 and finite", (double)p->scale);
  GLOC_REQUIRE(p->scale_start == 0.f || (p->scale_start >= p->scale && p->scale_start <= 3.4028235e38f), GLOC_ERR_INVALID,
               "robust scale_start = %g must be 0 or finite and >= scale = %g", (double)p->scale_start, (double)p->scale);
  GLOC_REQUIRE(p->scale_start == 0.f || (p->anneal > 0.f && p->anneal < 1.f), GLOC_ERR_INVALID,
               "robust anneal = %g outside (0, 1) with a schedule set", (double)p->anneal);
  return GLOC_OK;
}

}  // namespace robust
}  // namespace gloc

extern "C" {

void gloc_robust_default_params(gloc_robust_params* p) {
  if (!p) return;
  p->kind = GLOC_ROBUST_NONE;
  p->scale = 0.f;
  p->scale_start = 0.f;
  p->anneal = 0.f;
}

int gloc_robust_scale(const gloc_robust_params* prm, uint32_t pass, double* c) {
  GLOC_TRY(robust::check_params(prm));
  GLOC_REQUIRE(c, GLOC_ERR_INVALID, "null argument");
  *c = prm->kind == GLOC_ROBUST_NONE ? 0.0 : robust::scale_at(prm, pass);
  return GLOC_OK;
}

int gloc_robust_weight(const gloc_robust_params* prm, uint32_t pass, double s2, double* w) {
  GLOC_TRY(robust::check_params(prm));
  GLOC_REQUIRE(w, GLOC_ERR_INVALID, "null argument");
  if (prm->kind == GLOC_ROBUST_NONE) {
    *w = 1.0;
    return GLOC_OK;
  }
  const double c = robust::scale_at(prm, pass);
  *w = robust::weight_of(prm->kind, s2, c * c);
  return GLOC_OK;
}

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
