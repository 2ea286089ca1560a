// pairgraph.hpp -- what reg.hip (which owns the registration handle, the pair lists and the RANSAC stage's scoring and
// refit kernels) calls of pairgraph.hip: G1 - G3 of the correspondence-graph global registration.
#pragma once
#include "common.hpp"
#include "math3.hpp"

namespace gloc {
namespace pairgraph {

constexpr int MOMENTS = 16;  // per hypothesis: n, sum p [3], sum q [3], sum p q^T [9] (pairgraph_kernels.hpp PG_NV)

// The workspace budget: bit matrices and seed rows of as many jobs as fit are in flight at a time, the batch is walked in
// such groups (results do not depend on the grouping: a job's kernels read its own rows only).  A single job beyond it is
// refused (M ~ 90 000 pairs at the default 64 seeds).
constexpr size_t BUDGET_BYTES = 1ull << 30;

struct Ws {  // a registration handle's workspace, made on first use
  DevBuf bits, srow, sets;               // per group: [job][rows][words] x 8 B, [job][n_seeds][rows] x 4 B twice
  DevBuf score, degree, seeds, set_sizes;  // per batch: [job][rows], [job][rows], [job][n_seeds], [job][n_seeds]
  DevBuf moments;                          // per batch: [job][n_seeds][MOMENTS] fp64
  DevBuf counts;                           // [1]: gloc_reg_pair_graph's list length
};
void ws_free(Ws* w);

int check_params(const gloc_fpfh_graph_params* prm);

// The pair lists of a batch in the RANSAC stage's layout: counts[c] (device) pairs at pairs[(c * ld + i) * 2 + {0, 1}],
// none longer than m_max (known on the host).
struct Batch {
  const reg::f32x4* pairs;
  size_t ld;
  const uint32_t* counts;
  uint32_t n_jobs, m_max;
};

// G1 - G3 up to the fits for every job, enqueued on s: valid [job][n_seeds] and, left in w, the raw moments of every
// consensus set (w.moments: what the caller's solve turns into hypotheses), degree, score, seeds and set sizes.
// budget: bytes of matrices and seed rows in flight (0: BUDGET_BYTES).
int consensus_sets(hipStream_t s, Profiler& prof, Ws& w, const Batch& b, const gloc_fpfh_graph_params& prm, size_t budget, uint32_t* valid);

// G2 and G3's ranking for ONE bit matrix another stage has made (the pose graph's consistency matrix, pgo.hip): the same
// pg_score_kernel and pg_seeds_kernel, launched as a group of one job.  count (device, [1]): the matrix's side M <= rows;
// bits [rows][words], the bits past M zero.  score_matrix leaves score and degree [rows]; rank_seeds the n_seeds
// positions of largest key (any 64-bit key: the seed order is the kernel's), PG_NONE (0xFFFFFFFF) past M.
int score_matrix(hipStream_t s, const uint32_t* count, uint32_t rows, uint32_t words, unsigned long long* bits, unsigned long long* score,
                 uint32_t* degree);
int rank_seeds(hipStream_t s, const uint32_t* count, uint32_t rows, const unsigned long long* key, uint32_t n_seeds, uint32_t* seeds);

}  // namespace pairgraph
}  // namespace gloc
