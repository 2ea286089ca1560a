// fpfh.hip -- FPFH feature-based global registration (Rusu, Blodow & Beetz; pcl::FPFHEstimation in its k-nearest form,
// pcl::SampleConsensusPrerejective's idea of RANSAC over descriptor matches): the one stage that needs no initial guess
// in 3-D.  Host side of fpfh_kernels.hpp; tests/fpfh_ref.py is the contract.  The features live with the scans
// (scan_features.hip builds and keeps them through the functions here); the C entry points that match and register are in
// reg.hip, which owns the handle and runs its RANSAC stage on the pairs this file compacts.
#include <cmath>

#include "fpfh.hpp"
#include "fpfh_kernels.hpp"

using namespace gloc;
using namespace gloc::fpfh;

namespace gloc {
namespace fpfh {

static_assert(DIM == (int)FEAT_DIM, "one row layout");

void ws_free(Ws* w) { delete w; }

int check_params(const gloc_fpfh_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_TRY(check_support(Support::nearest(p->normal_k), SupportOf::NORMALS, SupportNames{"normal_k"}));
  GLOC_TRY(check_support(Support::nearest(p->feature_k), SupportOf::FEATURES, SupportNames{"feature_k"}));
  GLOC_REQUIRE(p->ransac_iters >= 1 && p->ransac_iters <= (1u << 20), GLOC_ERR_INVALID, "ransac_iters = %u outside [1, 2^20]",
               p->ransac_iters);
  GLOC_REQUIRE(p->inlier_thresh > 0.f, GLOC_ERR_INVALID, "inlier_thresh = %g must be > 0", (double)p->inlier_thresh);
  return GLOC_OK;
}

int check_radius_params(const gloc_fpfh_radius_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "radius params is null");
  GLOC_TRY(check_support(Support::normals_of(*p), SupportOf::NORMALS, SupportNames{nullptr, "normal_radius", "normal_max_nn", "normal_min_nn"}));
  GLOC_TRY(check_support(Support::features_of(*p), SupportOf::FEATURES, SupportNames{nullptr, "feature_radius", "feature_max_nn"}));
  GLOC_REQUIRE(p->reserved_ == 0, GLOC_ERR_INVALID, "reserved_ = %u must be 0", p->reserved_);
  return GLOC_OK;
}

int build_spfh(hipStream_t s, ground::NormalsScratch& w, const reg::f32x4* spts, const float* nrm_orig, uint32_t n, const Support& sup,
               uint8_t* spfh) {
  if (n == 0) return GLOC_OK;
  GLOC_TRY(ground::scan_lists(s, w, spts, n, sup));
  const bool wide = sup.by_radius();
  hipLaunchKernelGGL(wide ? spfh_wide_kernel : spfh_kernel, dim3(wide ? (n + 3) / 4 : (n + 255) / 256), dim3(256), 0, s, w.pts.as<f32x4>(),
                     nrm_orig, w.knn_idx.as<uint32_t>(), w.knn_d2.as<float>(), n, (int)sup.width(), spfh);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int build_fpfh(hipStream_t s, ground::NormalsScratch& w, const uint8_t* spfh, uint32_t n, const Support& sup, float* out) {
  if (n == 0) return GLOC_OK;
  const bool wide = sup.by_radius();
  hipLaunchKernelGGL(wide ? fpfh_wide_kernel : fpfh_kernel, dim3(wide ? (n + 3) / 4 : (n + 255) / 256), dim3(256), 0, s, spfh,
                     w.knn_idx.as<uint32_t>(), w.knn_d2.as<float>(), n, (int)sup.width(), out);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int reorder_rows(hipStream_t s, const reg::f32x4* spts, uint32_t n, const float* in, float* out, uint32_t width, bool to_sorted) {
  if (n == 0) return GLOC_OK;
  const size_t e = (size_t)n * width;
  hipLaunchKernelGGL(rows_reorder_kernel, dim3((unsigned)((e + 255) / 256)), dim3(256), 0, s, spts, n, in, out, width, to_sorted);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int match(hipStream_t s, Ws& w, const std::vector<MatchTask>& tasks) {
  uint32_t max_a = 0, max_b = 0;
  for (const MatchTask& t : tasks) {
    max_a = std::max(max_a, t.a_n);
    max_b = std::max(max_b, t.b_n);
  }
  if (tasks.empty() || max_a == 0 || max_b == 0) return GLOC_OK;
  GLOC_REQUIRE(tasks.size() <= 65535, GLOC_ERR_INVALID, "%zu searches in one launch", tasks.size());
  GLOC_TRY(w.tasks.ensure(sizeof(MatchTask) * tasks.size(), s));
  GLOC_HIP(hipMemcpyAsync(w.tasks.p, tasks.data(), sizeof(MatchTask) * tasks.size(), hipMemcpyHostToDevice, s));
  // The targets of a search are cut into slices (whole tiles) until the launch has ~4 work-groups per CU: one small job
  // alone would otherwise be 25 work-groups.  The slices meet in the keys' atomicMin, whose result no order changes.
  const uint32_t a_blocks = (max_a + MATCH_THREADS - 1) / MATCH_THREADS, tiles = (max_b + MATCH_TILE - 1) / MATCH_TILE;
  const size_t groups = (size_t)a_blocks * tasks.size();
  uint32_t slices = (uint32_t)std::min<size_t>(tiles, std::max<size_t>(1, (1024 + groups - 1) / groups));
  const uint32_t slice_tiles = (tiles + slices - 1) / slices;
  slices = (tiles + slice_tiles - 1) / slice_tiles;
  hipLaunchKernelGGL(fpfh_match_kernel, dim3(a_blocks, slices, (unsigned)tasks.size()), dim3(MATCH_THREADS), 0, s,
                     w.tasks.as<MatchTask>(), slice_tiles);
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipStreamSynchronize(s));  // (`tasks` is the caller's: the copy must have been consumed)
  return GLOC_OK;
}

int pairs(hipStream_t s, Ws& w, const std::vector<PairJob>& jobs, size_t ld, reg::f32x4* out_pairs, uint32_t* counts) {
  if (jobs.empty()) return GLOC_OK;
  GLOC_TRY(w.pjobs.ensure(sizeof(PairJob) * jobs.size(), s));
  GLOC_HIP(hipMemcpyAsync(w.pjobs.p, jobs.data(), sizeof(PairJob) * jobs.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(fpfh_pairs_kernel, dim3((unsigned)jobs.size()), dim3(1024), 0, s, w.pjobs.as<PairJob>(), ld, out_pairs, counts);
  GLOC_HIP(hipGetLastError());
  GLOC_HIP(hipStreamSynchronize(s));
  return GLOC_OK;
}

}  // namespace fpfh
}  // namespace gloc

extern "C" {

void gloc_fpfh_default_params(gloc_fpfh_params* p) {
  if (!p) return;
  p->normal_k = 10;       // registration/ground_estimator.cpp:79
  p->feature_k = 16;
  p->mutual = 1;
  p->ransac_iters = 3000;  // registration/loop_detector.cpp:257
  p->inlier_thresh = 0.6f;
  p->min_inlier_ratio = 0.f;
  p->ransac_confidence = 0.99f;
  p->reserved_ = 0;
  p->seed = 1234;
}

void gloc_fpfh_radius_default_params(gloc_fpfh_radius_params* p) {
  if (!p) return;
  p->normal_radius = 1.0f;   // 2 x the 0.5 m leaf the stage runs behind
  p->normal_max_nn = 30;
  p->normal_min_nn = 5;
  p->feature_radius = 2.5f;  // 5 x the leaf
  p->feature_max_nn = 100;
  p->reserved_ = 0;
}

}  // extern "C"
