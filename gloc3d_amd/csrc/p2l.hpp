// p2l.hpp -- what reg.hip (which owns the registration handle and the 1-NN passes) calls of p2l.hip.
#pragma once
#include "common.hpp"
#include "math3.hpp"

namespace gloc {
namespace p2l {

struct Ws;  // a handle's workspace for point-to-plane and generalized ICP (gn6.hpp; created on first use)
void ws_free(Ws* w);

struct TargetView {  // a job's target as the search indexes it
  const reg::f32x4* pts;
  const float* nrm;
  uint32_t n;
};

struct SourceView {  // a job's source in search order (idx.pts) with its normals in that order (null: none asked for)
  const reg::f32x4* pts;
  const float* nrm;
  uint32_t n;  // 0: a job without a target -- no work-group, no pair, the degenerate row of an empty target
};

// The handle's view for one batch: its stream, profiler and workspace slot, and the batch reg.hip has set up for the
// correspondence passes -- every job's source (the single-source entries repeat one), where job c's fp32 pose lives (what
// the search moves the source by; written here after every update), where a pass leaves its matches, and the pass itself.
struct Ctx {
  hipStream_t stream;
  Profiler* prof;
  Ws** ws;
  const SourceView* srcs;  // host [n_jobs]
  uint32_t n_jobs;
  float* pose_f32;     // device: 12 floats (R row-major 9, t 3) per job ...
  size_t pose_stride;  // ... this many floats apart
  const uint32_t* corr;  // device [job][ld], ld over the longest source: sorted source slot -> position in the target's search order
  const float* d2;
  size_t ld;
  int (*nn_pass)(void* self, bool warm);  // enqueues the exact 1-NN pass of every job at the current poses (null: no search)
  void* self;
};

// The robust half of a call (the _robust entries; include/gloc3d.h): the block, the pass the system form evaluates at and
// the outputs the plain entries do not have.  prm null or of kind NONE: the plain kernels.
struct RobustArgs {
  const gloc_robust_params* prm = nullptr;
  uint32_t pass = 0;
  float* out_weight = nullptr;  // [n]: the weights' sum over the count of the final evaluation
  double* out_wsum = nullptr;   // system form
  uint32_t kind() const { return prm ? prm->kind : (uint32_t)GLOC_ROBUST_NONE; }
};

int check_params(const gloc_p2l_params* prm);
// Refines every job from init_T ([n][16] or null: identity).  system36/g6/sum_r2/count non-null: ONE evaluation at init_T
// of job 0 instead (gloc_reg_p2l_system).  Returns after the results have been copied out.
int run(const Ctx& x, const TargetView* tgts, const float* init_T, const gloc_p2l_params* prm, float* out_T, float* out_rmse,
        uint32_t* out_iters, int* out_status, double* out_H36, double* out_g6, double* out_sum_r2, uint64_t* out_count,
        const RobustArgs& rb = RobustArgs());

}  // namespace p2l
}  // namespace gloc
