// fpfh.hpp -- what scan_features.hip (which owns the scans' features) and reg.hip (which owns the registration handle and
// the RANSAC stage) call of fpfh.hip.
#pragma once
#include <vector>

#include "common.hpp"
#include "ground_normals.hpp"
#include "math3.hpp"

namespace gloc {
namespace fpfh {

constexpr uint32_t FEAT_DIM = 33;        // floats per feature row (132 B)
constexpr uint32_t SPFH_BYTES = 36;      // per point: 33 counts, the pairs counted, padding
constexpr uint32_t MATCH_TILE_ROWS = 128;  // the matcher's target tile (tests size their shapes around it)

// One search of the matcher and one job of the pair compaction (fpfh_kernels.hpp has the field-by-field account).
struct MatchTask {
  const float* a_feat;
  const reg::f32x4* a_pts;
  const float* b_feat;
  const reg::f32x4* b_pts;
  unsigned long long* keys;
  uint32_t a_n, b_n;
};
struct PairJob {
  const unsigned long long* fwd;
  const unsigned long long* bwd;
  const float* src_xyz;
  const float* tgt_xyz;
  uint32_t n_src, n_tgt;
  // keypoint-restricted matching (I4): the keys are by keypoint RANK, and these lists turn a rank into the original index
  // whose xyz is fetched (null: the keys are by original index already)
  const uint32_t* src_map = nullptr;
  const uint32_t* tgt_map = nullptr;
};

struct Ws {  // a registration handle's workspace, made on first use
  DevBuf keys, tasks, pjobs, counts, feat_a, feat_b;
};
void ws_free(Ws* w);

int check_params(const gloc_fpfh_params* prm);
int check_radius_params(const gloc_fpfh_radius_params* prm);

// SPFH of the n points of `spts` (the store's sorted points) from their neighbour lists of `sup`, which this builds into w
// (ground::scan_lists), and the normals `nrm_orig` (original order): spfh [n][SPFH_BYTES] by original index.  Enqueued on s.
int build_spfh(hipStream_t s, ground::NormalsScratch& w, const reg::f32x4* spts, const float* nrm_orig, uint32_t n, const Support& sup,
               uint8_t* spfh);
// ... and the FPFH rows from them and the same lists (still in w): out [n][FEAT_DIM] by original index.  Both run a thread
// per point over k-NN lists and the wide-list kernels, a wave per point, over radius lists.
int build_fpfh(hipStream_t s, ground::NormalsScratch& w, const uint8_t* spfh, uint32_t n, const Support& sup, float* out);
// Rows of `width` floats between original order and the order of the sorted points.
int reorder_rows(hipStream_t s, const reg::f32x4* spts, uint32_t n, const float* in, float* out, uint32_t width, bool to_sorted);

// The searches `tasks` in one launch (their keys preset to all ones by the caller), then -- pairs() -- the kept matches of
// every job compacted into the RANSAC stage's layout, counts[job] pairs each.
int match(hipStream_t s, Ws& w, const std::vector<MatchTask>& tasks);
int pairs(hipStream_t s, Ws& w, const std::vector<PairJob>& jobs, size_t ld, reg::f32x4* out_pairs, uint32_t* counts);

}  // namespace fpfh
}  // namespace gloc
