// vgicp.hpp -- what reg.hip (which owns the registration handle) calls of vgicp.hip.
#pragma once
#include "common.hpp"
#include "p2l.hpp"  // the Gauss-Newton workspace the refinements share (gn6.hpp)
#include "scan_store.hpp"

namespace gloc {
namespace vgicp {

struct Ws;  // a handle's voxel maps and poses (created on first use)
void ws_free(Ws* w);

// The handle's view: its store, stream, profiler and the two workspace slots.
struct Ctx {
  gloc_scan_store* store;
  hipStream_t stream;
  Profiler* prof;
  Ws** ws;
  p2l::Ws** gn;
};

int check_params(const gloc_vgicp_params* prm);
// Refines n jobs from init_T ([n][16] or null: identity).  `pairs` false: the source scan src_ids[0] against n target scans;
// true: row c is (src_ids[c], tgt_ids[c]), 0xFFFFFFFF for "no target" (the row of an empty target), the ids checked before
// anything is enqueued.  Any of the last four non-null: ONE evaluation at init_T of job 0 instead (gloc_reg_vgicp_system).
// Returns after the results have been copied out.
int run(const Ctx& x, const uint32_t* src_ids, bool pairs, const uint32_t* tgt_ids, size_t n, const float* init_T, const gloc_vgicp_params* prm,
        float* out_T, float* out_rmse, uint32_t* out_iters, int* out_status, double* out_H36, double* out_g6, double* out_sum,
        uint64_t* out_count, const p2l::RobustArgs& rb = p2l::RobustArgs());
int voxels(const Ctx& x, uint32_t scan_id, const gloc_vgicp_params* prm, size_t capacity, int32_t* out_key3, uint32_t* out_count,
           double* out_mean3, double* out_nn6, size_t* n_voxels);

}  // namespace vgicp
}  // namespace gloc
