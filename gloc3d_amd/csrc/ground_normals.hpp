// ground_normals.hpp -- the neighbourhood support of a scan's normals and features, and the ground module's neighbour-list
// and normal kernels (ground_kernels.hpp, radius_kernels.hpp, compiled in ground.hip) run over a whole resident scan: what
// scan_features.hip calls to give a scan its per-point normals and fpfh.hip to start the features from.
#pragma once
#include "common.hpp"
#include "math3.hpp"

namespace gloc {

// The neighbourhood a point's normal or feature is computed from: none, the k nearest points, or every point within r --
// the max_nn nearest of them, and no normal where they are fewer than min_nn (0 for features; include/gloc3d.h R1 - R3).
// What a scan's normals and features are tagged with, and what every layer below the C entries is asked for.
struct Support {
  uint32_t k = 0;
  float r = 0.f;
  uint32_t max_nn = 0, min_nn = 0;
  static Support nearest(uint32_t k) { return Support{k, 0.f, 0u, 0u}; }
  static Support within(float r, uint32_t max_nn, uint32_t min_nn = 0) { return Support{0u, r, max_nn, min_nn}; }
  static Support normals_of(const gloc_fpfh_radius_params& p) { return within(p.normal_radius, p.normal_max_nn, p.normal_min_nn); }
  static Support features_of(const gloc_fpfh_radius_params& p) { return within(p.feature_radius, p.feature_max_nn); }
  bool by_radius() const { return k == 0 && (r != 0.f || max_nn != 0 || min_nn != 0); }
  bool none() const { return k == 0 && !by_radius(); }
  uint32_t width() const { return by_radius() ? max_nn : k; }  // the row length of the lists
  // (nothing is "built from" no support: none equals nothing, itself included)
  bool operator==(const Support& o) const { return !none() && k == o.k && r == o.r && max_nn == o.max_nn && min_nn == o.min_nn; }
};

// The ranges of a support, by what is computed from it: normals k in [3, 16] or min_nn in [4, max_nn]; features k in
// [4, 16] or max_nn >= 4; a bare search k in [3, 16] or max_nn >= 1 (its min_nn is not looked at); always r positive and
// finite and max_nn <= 128.  GLOC_ERR_INVALID with the offending field under the name its caller knows it by; a caller that
// names no k asks for a radius support (and an all-zero one is told about its r).
enum class SupportOf { NORMALS, FEATURES, SEARCH };
struct SupportNames {
  const char *k, *r, *max_nn, *min_nn;
};
int check_support(const Support& s, SupportOf what, const SupportNames& names);

namespace ground {

// scan_lists cuts the sorted points into chunks of this many and leaves one box per chunk in cbox_lo / cbox_hi (corners):
// what a kernel that sweeps the same chunks after it (iss_kernels.hpp) goes by.
constexpr int LIST_CHUNK = 64;

struct NormalsScratch {
  DevBuf pts, knn_idx, knn_d2, knn_cnt, cbox_lo, cbox_hi, bins, hist;
};

// The exact neighbour lists of the m points of `spts` (any spatially coherent order: x, y, z, bits(original index)) within
// the cloud, self included, ascending (d2, index): w.knn_idx / w.knn_d2 [m][sup.width()] by ORIGINAL index, entries a list
// cannot fill 0xFFFFFFFF / FLT_MAX, and w.pts the points in original order.  The k nearest, or (R1 of include/gloc3d.h) the
// max_nn nearest of those with d2 <= r * r, and then w.knn_cnt [m] the size of the whole neighbourhood.  What scan_normals
// and the FPFH features (fpfh.hip) both start from.  Enqueued on s; the lists take m x width x 8 bytes of w, grown on demand.
int scan_lists(hipStream_t s, NormalsScratch& w, const reg::f32x4* spts, uint32_t m, const Support& sup);

// Stable compaction of the indices whose byte flag is set (the two tiled kernels of ground_kernels.hpp): sel[0 .. *count)
// = the i < n with flag[i] != 0, ascending; n >= 1; tile_cnt: scratch, grown on demand.  Enqueued on s.
int select_flagged(hipStream_t s, const uint8_t* flag, uint32_t n, DevBuf& tile_cnt, uint32_t* sel, uint32_t* count);

// The chunks and boxes of scan_lists alone, for a sweep that keeps no lists (cluster_kernels.hpp): w.cbox_lo / w.cbox_hi
// of the ceil(m / LIST_CHUNK) chunks of `spts`.  Enqueued on s.
int scan_chunk_boxes(hipStream_t s, NormalsScratch& w, const reg::f32x4* spts, uint32_t m);

// Normals of the m points of `spts` from those lists, as gloc_ground_normals computes them from a list -- none (zero) where
// a radius list holds fewer than min_nn entries; out_normals [m][3] in ORIGINAL order (device).  Enqueued on s.
int scan_normals(hipStream_t s, NormalsScratch& w, const reg::f32x4* spts, uint32_t m, const Support& sup, float* out_normals);

}  // namespace ground
}  // namespace gloc
