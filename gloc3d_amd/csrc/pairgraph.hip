// pairgraph.hip -- correspondence-graph global registration on a match list (the second-order compatibility of SC2-PCR,
// Chen et al. 2022; TEASER's length invariant): two correct matches keep the distance between their points, two wrong
// ones almost never do, so the consistent set is read off a graph over the matches instead of being sampled.  Host side
// of pairgraph_kernels.hpp; tests/pairgraph_ref.py is the contract.  The C entry points are in reg.hip, which owns the
// handle, solves the fits from the moments made here and scores and refits them with the RANSAC stage's kernels.
#include "pairgraph.hpp"

#include <algorithm>

#include "pairgraph_kernels.hpp"

using namespace gloc;
using namespace gloc::pairgraph;

namespace gloc {
namespace pairgraph {

void ws_free(Ws* w) { delete w; }

int check_params(const gloc_fpfh_graph_params* p) {
  GLOC_REQUIRE(p, GLOC_ERR_INVALID, "params is null");
  GLOC_REQUIRE(p->normal_k >= 3 && p->normal_k <= 16, GLOC_ERR_INVALID, "normal_k = %u outside [3, 16]", p->normal_k);
  GLOC_REQUIRE(p->feature_k >= 4 && p->feature_k <= 16, GLOC_ERR_INVALID, "feature_k = %u outside [4, 16]", p->feature_k);
  GLOC_REQUIRE(p->n_seeds >= 1 && p->n_seeds <= 1024, GLOC_ERR_INVALID, "n_seeds = %u outside [1, 1024]", p->n_seeds);
  GLOC_REQUIRE(p->compat_thresh > 0.f, GLOC_ERR_INVALID, "compat_thresh = %g must be > 0", (double)p->compat_thresh);
  GLOC_REQUIRE(p->inlier_thresh > 0.f, GLOC_ERR_INVALID, "inlier_thresh = %g must be > 0", (double)p->inlier_thresh);
  GLOC_REQUIRE(p->theta_num >= 1 && p->theta_num <= p->theta_den, GLOC_ERR_INVALID, "theta_num / theta_den = %u / %u outside (0, 1]",
               p->theta_num, p->theta_den);
  return GLOC_OK;
}

static_assert(PG_NV == MOMENTS, "one layout of a set's moments");

int consensus_sets(hipStream_t s, Profiler& prof, Ws& w, const Batch& b, const gloc_fpfh_graph_params& prm, size_t budget, uint32_t* valid) {
  const uint32_t S = prm.n_seeds, n_jobs = b.n_jobs;
  if (n_jobs == 0) return GLOC_OK;
  if (b.m_max == 0) {  // no pairs anywhere: no hypotheses
    GLOC_HIP(hipMemsetAsync(valid, 0, sizeof(uint32_t) * (size_t)S * n_jobs, s));
    return GLOC_OK;
  }
  const uint32_t rows = b.m_max, words = (rows + 63u) / 64u;
  const size_t per_job = (size_t)rows * words * 8 + 2 * (size_t)S * rows * 4;
  GLOC_REQUIRE(per_job <= BUDGET_BYTES, GLOC_ERR_NOMEM, "a list of %u pairs needs %zu bytes of graph workspace, more than %zu", rows, per_job,
               BUDGET_BYTES);
  const uint32_t group = (uint32_t)std::min<size_t>(n_jobs, std::max<size_t>(1, (budget ? budget : BUDGET_BYTES) / per_job));
  GLOC_TRY(w.bits.ensure((size_t)group * rows * words * 8, s));
  GLOC_TRY(w.srow.ensure((size_t)group * S * rows * 4, s));
  GLOC_TRY(w.sets.ensure((size_t)group * S * rows * 4, s));
  GLOC_TRY(w.score.ensure((size_t)n_jobs * rows * 8, s));
  GLOC_TRY(w.degree.ensure((size_t)n_jobs * rows * 4, s));
  GLOC_TRY(w.seeds.ensure((size_t)n_jobs * S * 4, s));
  GLOC_TRY(w.set_sizes.ensure((size_t)n_jobs * S * 4, s));
  GLOC_TRY(w.moments.ensure((size_t)n_jobs * S * MOMENTS * sizeof(double), s));
  uint32_t lanes_per_row = 1;
  while (lanes_per_row < std::min(words, 64u)) lanes_per_row <<= 1;
  const double thr = (double)prm.compat_thresh;
  for (uint32_t j0 = 0; j0 < n_jobs; j0 += group) {
    const uint32_t nj = std::min(group, n_jobs - j0);
    const Group g{b.pairs, b.ld, b.counts, j0, rows, words, w.bits.as<unsigned long long>()};
    {
      ProfScope ps(prof, "pg_matrix", s);
      hipLaunchKernelGGL(pg_matrix_kernel, dim3(words, (rows + PG_MAT_ROWS - 1) / PG_MAT_ROWS, nj), dim3(PG_THREADS), 0, s, g, thr);
      GLOC_HIP(hipGetLastError());
    }
    {
      ProfScope ps(prof, "pg_score", s);
      hipLaunchKernelGGL(pg_score_kernel, dim3((rows + PG_WAVES - 1) / PG_WAVES, nj), dim3(PG_THREADS), sizeof(unsigned long long) * PG_WAVES * words, s,
                         g, lanes_per_row, w.score.as<unsigned long long>(), w.degree.as<uint32_t>());
      GLOC_HIP(hipGetLastError());
    }
    {
      ProfScope ps(prof, "pg_seeds", s);
      hipLaunchKernelGGL(pg_seeds_kernel, dim3(nj), dim3(PG_THREADS), 0, s, b.counts, j0, rows, w.score.as<unsigned long long>(), S,
                         w.seeds.as<uint32_t>());
      hipLaunchKernelGGL(pg_seed_sets_kernel, dim3(S, nj), dim3(PG_THREADS), sizeof(unsigned long long) * words, s, g, w.seeds.as<uint32_t>(), S,
                         prm.theta_num, prm.theta_den, w.srow.as<uint32_t>(), w.sets.as<uint32_t>(), w.set_sizes.as<uint32_t>());
      GLOC_HIP(hipGetLastError());
    }
    {
      ProfScope ps(prof, "pg_fit", s);
      hipLaunchKernelGGL(pg_moments_kernel, dim3(S, nj), dim3(PG_THREADS), 0, s, g, w.sets.as<uint32_t>(), w.set_sizes.as<uint32_t>(), S,
                         w.moments.as<double>(), valid);
      GLOC_HIP(hipGetLastError());
    }
  }
  return GLOC_OK;
}

int score_matrix(hipStream_t s, const uint32_t* count, uint32_t rows, uint32_t words, unsigned long long* bits, unsigned long long* score,
                 uint32_t* degree) {
  uint32_t lanes_per_row = 1;
  while (lanes_per_row < std::min(words, 64u)) lanes_per_row <<= 1;
  const Group g{nullptr, 0, count, 0u, rows, words, bits};  // (the score kernel reads counts, rows, words and bits only)
  hipLaunchKernelGGL(pg_score_kernel, dim3((rows + PG_WAVES - 1) / PG_WAVES, 1), dim3(PG_THREADS), sizeof(unsigned long long) * PG_WAVES * words, s, g,
                     lanes_per_row, score, degree);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

int rank_seeds(hipStream_t s, const uint32_t* count, uint32_t rows, const unsigned long long* key, uint32_t n_seeds, uint32_t* seeds) {
  hipLaunchKernelGGL(pg_seeds_kernel, dim3(1), dim3(PG_THREADS), 0, s, count, 0u, rows, key, n_seeds, seeds);
  GLOC_HIP(hipGetLastError());
  return GLOC_OK;
}

}  // namespace pairgraph
}  // namespace gloc

extern "C" {

void gloc_fpfh_graph_default_params(gloc_fpfh_graph_params* p) {
  if (!p) return;
  p->normal_k = 10;
  p->feature_k = 16;
  p->mutual = 1;
  p->n_seeds = 64;
  p->compat_thresh = 0.6f;
  p->inlier_thresh = 0.6f;
  p->min_inlier_ratio = 0.f;
  p->theta_num = 1;
  p->theta_den = 2;
  p->reserved_ = 0;
}

}  // extern "C"
