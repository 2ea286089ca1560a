// ground_normals.hpp -- the ground module's k-NN and normal kernels (ground_kernels.hpp, compiled in ground.hip) run over
// a whole resident scan: what scan_store.hip calls to give a scan its per-point normals.
#pragma once
#include "common.hpp"
#include "math3.hpp"

namespace gloc {
namespace ground {

struct NormalsScratch {
  DevBuf pts, knn_idx, knn_d2, knn_cnt, cbox_lo, cbox_hi, bins, hist;
};

// The exact k-NN lists of the m points of `spts` (any spatially coherent order: x, y, z, bits(original index)) within the
// cloud, self included, ascending (d2, index): w.knn_idx / w.knn_d2 [m][k] by ORIGINAL index, entries a list cannot fill
// 0xFFFFFFFF / FLT_MAX, and w.pts the points in original order.  What scan_normals and the FPFH features (fpfh.hip) both
// start from.  Enqueued on s; k in [3, 16].
int scan_knn(hipStream_t s, NormalsScratch& w, const reg::f32x4* spts, uint32_t m, uint32_t k);

// Normals of the m points of `spts` (any spatially coherent order: x, y, z, bits(original index)) from their k nearest
// neighbours within the cloud, as gloc_ground_normals computes them; out_normals [m][3] in ORIGINAL order (device).
// Enqueued on s; k in [3, 16].
int scan_normals(hipStream_t s, NormalsScratch& w, const reg::f32x4* spts, uint32_t m, uint32_t k, float* out_normals);

// The exact radius lists of the m points of `spts` within the cloud (R1 of include/gloc3d.h): every point with d2 <= r * r,
// self included, the max_nn nearest in ascending (d2, index) -- w.knn_idx / w.knn_d2 [m][max_nn] by ORIGINAL index, padded
// as scan_knn pads, w.knn_cnt [m] the size of the whole neighbourhood, w.pts the points in original order.  Enqueued on s;
// r > 0 and finite, max_nn in [1, 128].  The lists take m x max_nn x 8 bytes of w, grown on demand.
int scan_radius(hipStream_t s, NormalsScratch& w, const reg::f32x4* spts, uint32_t m, float r, uint32_t max_nn);

// Normals from the radius lists of (r, max_nn): none (zero) where a list holds fewer than min_nn entries, else what
// scan_normals computes from that list; out_normals [m][3] in ORIGINAL order (device).  Enqueued on s.
int scan_normals_radius(hipStream_t s, NormalsScratch& w, const reg::f32x4* spts, uint32_t m, float r, uint32_t max_nn, uint32_t min_nn,
                        float* out_normals);

}  // namespace ground
}  // namespace gloc
