// vmap.hpp -- what reg.hip (which owns the registration handle) calls of vmap.hip: the handle's resident voxel maps
// (include/gloc3d.h: M1 - M8) -- made, filled, pruned, exported -- and the voxelized refinement against them.
#pragma once
#include "common.hpp"
#include "scan_store.hpp"
#include "vgicp.hpp"

namespace gloc {
namespace vmap {

struct Set;  // a handle's maps and the scratch of their inserts and prunes (created on first use)
void set_free(Set* s);

// The handle's view: its store, stream, profiler and the slot of its maps.
struct Ctx {
  gloc_scan_store* store;
  hipStream_t stream;
  Profiler* prof;
  Set** set;
};

int check_params(const gloc_vmap_params* prm);
int create(const Ctx& x, const gloc_vmap_params* prm, uint32_t* out_map_id);
int destroy(const Ctx& x, uint32_t map_id);
// is map_id a map of the handle?  (GLOC_ERR_INVALID and the message if not; nothing is enqueued)
int check_id(const Ctx& x, uint32_t map_id);
// The single inserts of the list in order (M2 - M4); T [n][16] or null.  Every id is checked before anything is enqueued.
int insert(const Ctx& x, uint32_t map_id, const uint32_t* scan_ids, size_t n, const float* T);
int prune(const Ctx& x, uint32_t map_id, const float* center3, float max_dist, uint32_t max_age, uint32_t* out_removed);
int info(const Ctx& x, uint32_t map_id, gloc_vmap_info* out);
int voxels(const Ctx& x, uint32_t map_id, size_t capacity, int32_t* out_key3, uint32_t* out_count, double* out_mean3, double* out_nn6,
           uint32_t* out_stamp, size_t* n_voxels);
// vgicp::run with row j's target the map c.tgt_ids[j] (0xFFFFFFFF: none) instead of a scan's voxels (M7): the ids, the
// resolution and min_points are checked before anything is enqueued.
int refine(const Ctx& x, const vgicp::Ctx& v, const gn6::Call& c, const gloc_vgicp_params* prm);

}  // namespace vmap
}  // namespace gloc
