// p2l_kernels.hpp -- the accumulate kernel of the point-to-plane ICP refinement (gfx950).  tests/p2l_ref.py is the contract.
//
//   p2l_accum_kernel   one lane per source point (sorted slot): p = R s + t in fp32 as the search moved it, the matched
//                      target point and its normal, r = n.(p - q), J = [p x n ; n]; the 29 sums of a pass (21 entries of
//                      the upper triangle of J J^T, 6 of J r, r^2, the count) in fp64, one partial per work-group
//
// KIND (robust.hpp; 0: none, the plain entries' instantiation, whose arithmetic is what it was before there were kinds):
// the lane that owns the pair takes s2 = r^2 and the weight w of the pass's scale, and forms its 27 contributions to H
// and g from w J in place of one J -- (w J) J^T and (w J) r -- leaving r^2 and the count alone; slot 29 gets the weight.
//
// The reduction of those sums, the solve kernel and the note on registers are in gn6_kernels.hpp, shared with the
// generalized ICP.  The correspondences are the registration's own exact 1-NN pass (reg.hip: launch_nn), unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gn6_kernels.hpp"
#include "math3.hpp"  // f32x4, xform

namespace gloc {
namespace p2l {

using reg::f32x4;
using gn6::ACC_THREADS;
using gn6::NSLOT;
using gn6::NSUM;
using gn6::State;
using gn6::Target;

template <int KIND>
__global__ __launch_bounds__(ACC_THREADS) void p2l_accum_kernel(const gn6::Source* __restrict__ srcs, const Target* __restrict__ tgts,
                                                                const float* __restrict__ pose_f32, size_t pose_stride /* floats */,
                                                                const State* __restrict__ states, const uint32_t* __restrict__ corr,
                                                                const float* __restrict__ d2in, size_t ld, float gate2, bool skip_stopped,
                                                                double* __restrict__ partials /* [srcs[job].row0 + block][NSLOT] */,
                                                                gn6::Scale2 sc) {
  __shared__ double red[ACC_THREADS / 64][NSLOT];
  const uint32_t job = blockIdx.y;
  const gn6::Source S = srcs[job];
  if (blockIdx.x >= S.n_blk) return;                // (uniform: the grid is as wide as the batch's longest source)
  if (skip_stopped && states[job].stopped) return;  // (uniform; the solve does not read a stopped job's partials)
  const uint32_t i = blockIdx.x * ACC_THREADS + threadIdx.x;
  double v[NSLOT];
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) v[k] = 0.0;
  if (i < S.n) {
    const Target T = tgts[job];
    const uint32_t j = corr[(size_t)job * ld + i];
    const float d2 = d2in[(size_t)job * ld + i];
    // (d2 - d2 == 0: finite)
    if (j < T.n && d2 - d2 == 0.f && (!(gate2 > 0.f) || d2 <= gate2)) {
      const float nx = T.nrm[3 * (size_t)j], ny = T.nrm[3 * (size_t)j + 1], nz = T.nrm[3 * (size_t)j + 2];
      if (nx != 0.f || ny != 0.f || nz != 0.f) {
        float Tf[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Tf[k] = pose_f32[(size_t)job * pose_stride + k];
        const f32x4 s = S.pts[i];
        const f32x4 q = T.pts[j];
        float px, py, pz;
        reg::xform(Tf, s.x, s.y, s.z, px, py, pz);
        const double P[3] = {(double)px, (double)py, (double)pz};
        const double N[3] = {(double)nx, (double)ny, (double)nz};
        const double r = (N[0] * (P[0] - (double)q.x) + N[1] * (P[1] - (double)q.y)) + N[2] * (P[2] - (double)q.z);
        double J[6];
        reg::cross3(P, N, J);
        J[3] = N[0]; J[4] = N[1]; J[5] = N[2];
        v[27] = r * r;
        v[28] = 1.0;
        double Jw[6];  // w J: the weight rides on one factor of J J^T and of J r (the plain kernel: J itself)
        if (KIND != GLOC_ROBUST_NONE) {
          const double w = robust::weight<KIND>(v[27], gn6::scale2_of(sc, states[job]));
#pragma unroll
          for (int a = 0; a < 6; ++a) Jw[a] = J[a] * w;
          v[gn6::WSLOT] = w;
        } else {
#pragma unroll
          for (int a = 0; a < 6; ++a) Jw[a] = J[a];
        }
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) v[e++] = Jw[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) v[21 + a] = Jw[a] * r;
      }
    }
  }
  gn6::reduce_store(v, red, partials + ((size_t)S.row0 + blockIdx.x) * NSLOT);
}

}  // namespace p2l
}  // namespace gloc
