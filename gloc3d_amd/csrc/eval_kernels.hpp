// eval_kernels.hpp -- the accumulate kernel of the point-to-point evaluation of registered pairs (gfx950).
// tests/eval_ref.py is the contract (V1 - V6 of include/gloc3d.h).
//
//   eval_accum_kernel   one lane per source point (sorted slot): p = R s + t in fp32 as the search moved it, the matched
//                       target point q, e = p - q, J = [-[p]x , I]; the 29 sums of the evaluation (21 entries of the upper
//                       triangle of J^T J, 6 of J^T e, |e|^2, the count) in fp64, one partial per work-group
//
// The layout of the sums is the refinements' (gn6_kernels.hpp), so the reduction (reduce_store), the partial rows and the
// index-order sum of solve_kernel in evaluation mode are theirs, unchanged.  No normals, no robust kinds, no atomics.
// The entries of J are fp32 values widened, so every product that goes into J^T J is exact in fp64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gn6_kernels.hpp"
#include "math3.hpp"  // f32x4, xform

namespace gloc {
namespace eval {

using reg::f32x4;
using gn6::ACC_THREADS;
using gn6::NSLOT;
using gn6::Target;

__global__ __launch_bounds__(ACC_THREADS) void eval_accum_kernel(const gn6::Source* __restrict__ srcs, const Target* __restrict__ tgts,
                                                                 const float* __restrict__ pose_f32, size_t pose_stride /* floats */,
                                                                 const uint32_t* __restrict__ corr, const float* __restrict__ d2in,
                                                                 size_t ld, float gate2,
                                                                 double* __restrict__ partials /* [srcs[job].row0 + block][NSLOT] */) {
  __shared__ double red[ACC_THREADS / 64][NSLOT];
  const uint32_t job = blockIdx.y;
  const gn6::Source S = srcs[job];
  if (blockIdx.x >= S.n_blk) return;  // (uniform: the grid is as wide as the batch's longest source)
  const uint32_t i = blockIdx.x * ACC_THREADS + threadIdx.x;
  double v[NSLOT];
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) v[k] = 0.0;
  if (i < S.n) {
    const Target T = tgts[job];
    const uint32_t j = corr[(size_t)job * ld + i];
    const float d2 = d2in[(size_t)job * ld + i];
    // V3 (d2 - d2 == 0: finite)
    if (j < T.n && d2 - d2 == 0.f && d2 <= gate2) {
      float Tf[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) Tf[k] = pose_f32[(size_t)job * pose_stride + k];
      const f32x4 s = S.pts[i];
      const f32x4 q = T.pts[j];
      float pxf, pyf, pzf;
      reg::xform(Tf, s.x, s.y, s.z, pxf, pyf, pzf);
      const double px = (double)pxf, py = (double)pyf, pz = (double)pzf;
      const double ex = px - (double)q.x, ey = py - (double)q.y, ez = pz - (double)q.z;
      // J^T J with J = [-[p]x , I]: the columns of -[p]x are (0, -pz, py), (pz, 0, -px), (-py, px, 0)
      v[0] = py * py + pz * pz;
      v[1] = -(px * py);
      v[2] = -(px * pz);
      v[4] = -pz;
      v[5] = py;
      v[6] = px * px + pz * pz;
      v[7] = -(py * pz);
      v[8] = pz;
      v[10] = -px;
      v[11] = px * px + py * py;
      v[12] = -py;
      v[13] = px;
      v[15] = 1.0;
      v[18] = 1.0;
      v[20] = 1.0;
      // J^T e = (p x e, e)
      v[21] = py * ez - pz * ey;
      v[22] = pz * ex - px * ez;
      v[23] = px * ey - py * ex;
      v[24] = ex;
      v[25] = ey;
      v[26] = ez;
      v[27] = (ex * ex + ey * ey) + ez * ez;
      v[28] = 1.0;
    }
  }
  gn6::reduce_store(v, red, partials + ((size_t)S.row0 + blockIdx.x) * NSLOT);
}

}  // namespace eval
}  // namespace gloc
