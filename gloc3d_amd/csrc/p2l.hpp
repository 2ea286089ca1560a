// p2l.hpp -- what the Gauss-Newton refinements (p2l.hip, gicp.hip, vgicp.hip) share on the host with reg.hip, which owns
// the registration handle and the 1-NN passes: the description of a call (gn6::Call), the handle's view for one batch
// (Ctx) and the entry points of p2l.hip.
#pragma once
#include "common.hpp"
#include "math3.hpp"

namespace gloc {
namespace gn6 {

// A job's target as the point-based accumulate kernels take it (p2l_kernels.hpp, gicp_kernels.hpp): the scan as the search
// indexes it.  reg.hip fills the table; n = 0 (and null pointers): a job without a target.
struct Target {
  const reg::f32x4* pts;  // the search order: x, y, z, bits(original index)
  const float* nrm;       // normals in that order, packed; zero = none
  uint32_t n, pad_;
};

// One call of a refinement entry, whatever its cost function: the jobs, where the results go and the robust half.  A C
// entry of reg.hip fills one; everything below it -- refine_entry, run_p2l / run_gicp, run_refine, vgicp::run, p2l::run,
// gicp::run, gn6::run -- takes it beside the method's own parameter block.
struct Call {
  // the jobs: the ONE source src_ids[0] against n targets, or with `pairs` row c is (src_ids[c], tgt_ids[c]), 0xFFFFFFFF in
  // tgt_ids for "no target"; init_T [n][16] or null: identity
  const uint32_t* src_ids = nullptr;
  bool pairs = false;
  const uint32_t* tgt_ids = nullptr;
  size_t n = 0;
  const float* init_T = nullptr;
  // false: every job is refined and the batch outputs [n] are written (out_T is asked for, the others may be null);
  // true: ONE evaluation of every job at its init_T into the system outputs, [n] rows each (all asked for; out_wsum by a
  // robust entry): n = 1 from the single-pair entries, a list with `pairs`
  bool system = false;
  float *out_T = nullptr, *out_rmse = nullptr;
  uint32_t* out_iters = nullptr;
  int* out_status = nullptr;
  float* out_weight = nullptr;  // the weights' sum over the count of the final evaluation
  double *out_H36 = nullptr, *out_g6 = nullptr, *out_sum = nullptr;
  uint64_t* out_count = nullptr;
  double* out_wsum = nullptr;
  // the robust half (robust.hpp; include/gloc3d.h): null or of kind NONE: the plain kernels.  need_robust: the entry is a
  // _robust one, which refuses a null block; pass: the update the system form evaluates at
  const gloc_robust_params* robust = nullptr;
  bool need_robust = false;
  uint32_t pass = 0;
  uint32_t kind() const { return robust ? robust->kind : (uint32_t)GLOC_ROBUST_NONE; }
};

}  // namespace gn6

namespace p2l {

struct Ws;  // a handle's workspace for point-to-plane and generalized ICP (gn6.hpp; created on first use)
void ws_free(Ws* w);

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

int check_params(const gloc_p2l_params* prm);
// Refines every job of c, or evaluates every job once (c.system); tgts [x.n_jobs]: the jobs' targets as the search indexes
// them.  Returns after the results have been copied out.
int run(const Ctx& x, const gn6::Target* tgts, const gn6::Call& c, const gloc_p2l_params* prm);

}  // namespace p2l
}  // namespace gloc
