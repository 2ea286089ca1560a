// fgr.hip -- Fast Global Registration (Zhou, Park, Koltun, ECCV 2016) on a match list: a tuple test on the matches, then
// one graduated-non-convexity optimisation over the fixed correspondences with the Geman-McClure line process, its scale
// annealed from the clouds' extent down to the match distance.  No hypotheses, no scoring, no neighbour search behind
// the matcher.  Host side of fgr_kernels.hpp; tests/fgr_ref.py is the contract.  The C entry points are in reg.hip, which
// owns the handle and the pair lists.
#include "fgr.hpp"

#include <algorithm>
#include <cmath>

#include "fgr_kernels.hpp"

using namespace gloc;
using namespace gloc::fgr;

namespace gloc {
namespace fgr {

void ws_free(Ws* w) { delete w; }

int check_params(const gloc_fgr_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->normal_k >= 3 && p->normal_k <= 16, GLOC_ERR_INVALID, "normal_k = %u outside [3, 16]", p->normal_k);
  GLOC_REQUIRE(p->feature_k >= 4 && p->feature_k <= 16, GLOC_ERR_INVALID, "feature_k = %u outside [4, 16]", p->feature_k);
  GLOC_REQUIRE(p->tuple_tries <= (1u << 20), GLOC_ERR_INVALID, "tuple_tries = %u above 2^20", p->tuple_tries);
  GLOC_REQUIRE(p->max_tuples >= 1 && p->max_tuples <= (1u << 20), GLOC_ERR_INVALID, "max_tuples = %u outside [1, 2^20]", p->max_tuples);
  GLOC_REQUIRE(p->tuple_scale > 0.f && p->tuple_scale <= 1.f, GLOC_ERR_INVALID, "tuple_scale = %g outside (0, 1]", (double)p->tuple_scale);
  GLOC_REQUIRE(p->max_iters >= 1 && p->max_iters <= 1024, GLOC_ERR_INVALID, "max_iters = %u outside [1, 1024]", p->max_iters);
  GLOC_REQUIRE(p->anneal_every >= 1, GLOC_ERR_INVALID, "anneal_every = %u must be >= 1", p->anneal_every);
  GLOC_REQUIRE(p->anneal_div > 1.f && std::isfinite(p->anneal_div), GLOC_ERR_INVALID, "anneal_div = %g must be > 1 and finite",
               (double)p->anneal_div);
  GLOC_REQUIRE(p->max_corr_dist > 0.f && std::isfinite(p->max_corr_dist), GLOC_ERR_INVALID, "max_corr_dist = %g must be > 0 and finite",
               (double)p->max_corr_dist);
  GLOC_REQUIRE(p->inlier_thresh > 0.f, GLOC_ERR_INVALID, "inlier_thresh = %g must be > 0", (double)p->inlier_thresh);
  return GLOC_OK;
}

int enqueue(hipStream_t s, Profiler& prof, Ws& w, const Batch& b, const gloc_fgr_params& prm) {
  const uint32_t n_jobs = b.n_jobs;
  if (n_jobs == 0) return GLOC_OK;
  const uint32_t tries = prm.tuple_tries, words = (tries + 63u) / 64u;
  const size_t ld = std::max<size_t>(b.ld, 1);
  GLOC_TRY(w.bits.ensure(sizeof(unsigned long long) * std::max<size_t>((size_t)words * n_jobs, 1), s));
  GLOC_TRY(w.mult.ensure(sizeof(uint32_t) * ld * n_jobs, s));
  GLOC_TRY(w.act.ensure(sizeof(uint32_t) * ld * n_jobs, s));
  GLOC_TRY(w.results.ensure(sizeof(Result) * n_jobs, s));
  GLOC_HIP(hipMemsetAsync(w.mult.p, 0, sizeof(uint32_t) * ld * n_jobs, s));
  const Rule r{tries, prm.max_tuples, prm.max_iters, prm.anneal_every, (double)prm.tuple_scale, (double)prm.anneal_div,
               (double)prm.max_corr_dist * (double)prm.max_corr_dist, prm.inlier_thresh * prm.inlier_thresh, prm.seed};
  const JobIn* jobs = w.jobs.as<JobIn>();
  if (tries) {
    ProfScope ps(prof, "fgr_tuple", s);
    hipLaunchKernelGGL(tuple_kernel, dim3((tries + THREADS - 1) / THREADS, n_jobs), dim3(THREADS), 0, s, b.pairs, b.ld, jobs, r,
                       w.bits.as<unsigned long long>(), words);
    GLOC_HIP(hipGetLastError());
  }
  // the active pairs of a job: no more than its list, nor than three members of every kept tuple
  uint64_t most = b.m_max;
  if (tries) most = std::min<uint64_t>(most, 3ull * std::min(prm.max_tuples, tries));
  const uint32_t cap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(most, 1), LDS_CAP);
  const size_t lds = (size_t)ENTRY_BYTES * cap;
  if (!w.lds_attr) {
    GLOC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(gnc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(ENTRY_BYTES * LDS_CAP)));
    w.lds_attr = true;
  }
  {
    ProfScope ps(prof, "fgr_gnc", s);
    hipLaunchKernelGGL(gnc_kernel, dim3(n_jobs), dim3(THREADS), lds, s, b.pairs, b.ld, jobs, r, w.bits.as<unsigned long long>(), words, cap,
                       w.mult.as<uint32_t>(), w.act.as<uint32_t>(), w.results.as<Result>());
    GLOC_HIP(hipGetLastError());
  }
  return GLOC_OK;
}

}  // namespace fgr
}  // namespace gloc

extern "C" {

void gloc_fgr_default_params(gloc_fgr_params* p) {
  if (!p) return;
  p->normal_k = 10;
  p->feature_k = 16;
  p->mutual = 1;
  p->tuple_tries = 10000;
  p->max_tuples = 1000;
  p->tuple_scale = 0.9f;
  p->max_iters = 64;
  p->anneal_every = 4;
  p->anneal_div = 1.4f;
  p->max_corr_dist = 0.6f;
  p->inlier_thresh = 0.6f;
  p->min_inlier_ratio = 0.f;
  p->seed = 1234;
}

}  // extern "C"
