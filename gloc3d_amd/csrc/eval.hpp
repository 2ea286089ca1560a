// eval.hpp -- the point-to-point evaluation of registered pairs (gloc_reg_evaluate_pairs; eval.hip, eval_kernels.hpp) as
// reg.hip, which owns the handle and sets up the batch, sees it.
#pragma once
#include "common.hpp"
#include "p2l.hpp"

namespace gloc {
namespace eval {

struct Out {  // [n] rows each; any may be null
  float *fitness, *rmse;
  uint32_t* count;
  double *info36, *g6;
};

int check_params(const gloc_eval_params* prm);
// Evaluates every job of the batch x ONCE at its pose T + 16 c (null: the identity): one cold 1-NN pass over all jobs, one
// accumulate launch, the shared solve kernel in evaluation mode, one copy of all jobs' sums (gn6::run's system form).
// tgts [x.n_jobs]: the jobs' targets as the search indexes them (their normals are not read).  Returns after the
// results have been written.
int run(const p2l::Ctx& x, const gn6::Target* tgts, const float* T, const gloc_eval_params* prm, const Out& out);

}  // namespace eval
}  // namespace gloc
