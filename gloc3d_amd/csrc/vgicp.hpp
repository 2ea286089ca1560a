// vgicp.hpp -- what reg.hip (which owns the registration handle) calls of vgicp.hip: run() with the gn6::Call its entry
// filled and refine_entry has checked, and voxels().
#pragma once
#include "common.hpp"
#include "p2l.hpp"  // gn6::Call and the Gauss-Newton workspace the refinements share (gn6.hpp)
#include "scan_store.hpp"

namespace gloc {
namespace vgicp {

struct Ws;  // a handle's voxel maps and poses (created on first use)
void ws_free(Ws* w);
struct Target;  // a job's hash table and voxels as the accumulate kernel takes them (vgicp_kernels.hpp)

// The handle's view: its store, stream, profiler and the two workspace slots.
struct Ctx {
  gloc_scan_store* store;
  hipStream_t stream;
  Profiler* prof;
  Ws** ws;
  p2l::Ws** gn;
};

int check_params(const gloc_vgicp_params* prm);
// Refines every job of c, or evaluates job 0 once (c.system): the scans of the call resolved (reg::CallScans), a voxel map
// per distinct target, then gn6.hpp's loop.  Returns after the results have been copied out.
// resident (vmap.hip) not null: c is a pair list whose targets are NOT scans -- row j probes resident[j], a view into a map
// that outlives the call (hkey null: a row without a target); only the sources are resolved and no map is built.
int run(const Ctx& x, const gn6::Call& c, const gloc_vgicp_params* prm, const Target* resident = nullptr);
int voxels(const Ctx& x, uint32_t scan_id, const gloc_vgicp_params* prm, size_t capacity, int32_t* out_key3, uint32_t* out_count,
           double* out_mean3, double* out_nn6, size_t* n_voxels);

}  // namespace vgicp
}  // namespace gloc
