// gicp_kernels.hpp -- the accumulate kernel of the generalized (plane-to-plane) ICP refinement (gfx950).
// tests/gicp_ref.py is the contract.
//
//   gicp_accum_kernel  one lane per source point (sorted slot): p = R s + t in fp32 as the search moved it, the source's
//                      normal n_s at the slot, the matched target point q and its normal n_j; in fp64 m = R n_s,
//                      S = 2I - a (n_j n_j^T + m m^T) with a = 1 - plane_eps, M = S^-1, e = p - q, J = [-[p]x , I];
//                      the 29 sums of a pass (21 entries of the upper triangle of J^T M J, 6 of J^T M e, e^T M e, the
//                      count), one partial per work-group
//
// M is the symmetric adjugate of S over its determinant: 6 cofactors, one fp64 division.  For unit normals S has
// eigenvalues in [2 plane_eps, 2] -- the smallest where the two normals are parallel -- so the determinant is at least
// 8 plane_eps, far from zero in fp64 for any plane_eps above the normals' own fp32 rounding (1e-7).  With A = [p]x M (a cross product per column of M) the blocks of
// J^T M J are
//   ww = -A [p]x  (row i: p x A_i.),   wv = A,   vv = M,      and J^T M e = (p x M e ; M e).
// About 150 fp64 operations and one division per pair; the 1-NN search of the same pass is two orders above that.
//
// KIND (robust.hpp; 0: none, the plain entries' instantiation, whose arithmetic is what it was before there were kinds):
// the lane that owns the pair takes s2 = e^T M e from the adjugate -- (e^T adj e) / det -- and the weight w of the pass's
// scale, which then rides on M (w / det), so that the 27 contributions to H and g come out weighted; e^T M e (s2 itself)
// and the count are left alone; slot 29 gets the weight.  One more division (a square root with it for Huber) beside the
// pair's own.
//
// The reduction of the sums, the solve kernel and the note on registers are in gn6_kernels.hpp, shared with the
// point-to-plane refinement.  The correspondences are the registration's own exact 1-NN pass (reg.hip: launch_nn).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gn6_kernels.hpp"
#include "math3.hpp"  // f32x4, xform, cross3

namespace gloc {
namespace gicp {

using reg::f32x4;
using gn6::ACC_THREADS;
using gn6::NSLOT;
using gn6::NSUM;
using gn6::State;
using gn6::Target;

template <int KIND>
__global__ __launch_bounds__(ACC_THREADS) void gicp_accum_kernel(const gn6::Source* __restrict__ srcs, const Target* __restrict__ tgts,
                                                                 const float* __restrict__ pose_f32, size_t pose_stride /* floats */,
                                                                 const State* __restrict__ states, const uint32_t* __restrict__ corr,
                                                                 const float* __restrict__ d2in, size_t ld, float gate2, double a,
                                                                 bool skip_stopped,
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
    // (d2 - d2 == 0: finite, and then so is p)
    if (j < T.n && d2 - d2 == 0.f && (!(gate2 > 0.f) || d2 <= gate2)) {
      float Tf[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) Tf[k] = pose_f32[(size_t)job * pose_stride + k];
      const f32x4 s = S.pts[i];
      const f32x4 q = T.pts[j];
      float px, py, pz;
      reg::xform(Tf, s.x, s.y, s.z, px, py, pz);
      const double P[3] = {(double)px, (double)py, (double)pz};
      const double E[3] = {P[0] - (double)q.x, P[1] - (double)q.y, P[2] - (double)q.z};
      const double B[3] = {(double)T.nrm[3 * (size_t)j], (double)T.nrm[3 * (size_t)j + 1], (double)T.nrm[3 * (size_t)j + 2]};
      const double ns[3] = {(double)S.nrm[3 * (size_t)i], (double)S.nrm[3 * (size_t)i + 1], (double)S.nrm[3 * (size_t)i + 2]};
      double m[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) m[r] = ((double)Tf[3 * r] * ns[0] + (double)Tf[3 * r + 1] * ns[1]) + (double)Tf[3 * r + 2] * ns[2];
      // S = 2I - a (B B^T + m m^T), symmetric: xx xy xz yy yz zz
      const double sxx = 2.0 - a * (B[0] * B[0] + m[0] * m[0]), sxy = -a * (B[0] * B[1] + m[0] * m[1]);
      const double sxz = -a * (B[0] * B[2] + m[0] * m[2]), syy = 2.0 - a * (B[1] * B[1] + m[1] * m[1]);
      const double syz = -a * (B[1] * B[2] + m[1] * m[2]), szz = 2.0 - a * (B[2] * B[2] + m[2] * m[2]);
      const double cxx = syy * szz - syz * syz, cxy = sxz * syz - sxy * szz, cxz = sxy * syz - sxz * syy;
      const double cyy = sxx * szz - sxz * sxz, cyz = sxy * sxz - sxx * syz, czz = sxx * syy - sxy * sxy;
      double inv = 1.0 / ((sxx * cxx + sxy * cxy) + sxz * cxz);
      double s2 = 0.0;
      if (KIND != GLOC_ROBUST_NONE) {
        // s2 = e^T M e from the adjugate, before the weight rides on M
        const double ce[3] = {(cxx * E[0] + cxy * E[1]) + cxz * E[2], (cxy * E[0] + cyy * E[1]) + cyz * E[2],
                              (cxz * E[0] + cyz * E[1]) + czz * E[2]};
        s2 = ((E[0] * ce[0] + E[1] * ce[1]) + E[2] * ce[2]) * inv;
        const double w = robust::weight<KIND>(s2, gn6::scale2_of(sc, states[job]));
        inv = w * inv;
        v[gn6::WSLOT] = w;
      }
      const double M[3][3] = {{cxx * inv, cxy * inv, cxz * inv}, {cxy * inv, cyy * inv, cyz * inv}, {cxz * inv, cyz * inv, czz * inv}};
      double Me[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) Me[r] = (M[r][0] * E[0] + M[r][1] * E[1]) + M[r][2] * E[2];
      // A = [p]x M: column k is p x (column k of M) -- M is symmetric, so its row k
      double A[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double c[3];
        reg::cross3(P, M[k], c);
        A[0][k] = c[0]; A[1][k] = c[1]; A[2][k] = c[2];
      }
      double W[3][3];  // ww block: row i = p x (row i of A)
#pragma unroll
      for (int r = 0; r < 3; ++r) reg::cross3(P, A[r], W[r]);
      double gw[3];
      reg::cross3(P, Me, gw);
      // the upper triangle of the 6 x 6, row-major
      v[0] = W[0][0]; v[1] = W[0][1]; v[2] = W[0][2]; v[3] = A[0][0]; v[4] = A[0][1]; v[5] = A[0][2];
      v[6] = W[1][1]; v[7] = W[1][2]; v[8] = A[1][0]; v[9] = A[1][1]; v[10] = A[1][2];
      v[11] = W[2][2]; v[12] = A[2][0]; v[13] = A[2][1]; v[14] = A[2][2];
      v[15] = M[0][0]; v[16] = M[0][1]; v[17] = M[0][2];
      v[18] = M[1][1]; v[19] = M[1][2];
      v[20] = M[2][2];
      v[21] = gw[0]; v[22] = gw[1]; v[23] = gw[2];
      v[24] = Me[0]; v[25] = Me[1]; v[26] = Me[2];
      v[27] = KIND != GLOC_ROBUST_NONE ? s2 : (E[0] * Me[0] + E[1] * Me[1]) + E[2] * Me[2];
      v[28] = 1.0;
    }
  }
  gn6::reduce_store(v, red, partials + ((size_t)S.row0 + blockIdx.x) * NSLOT);
}

}  // namespace gicp
}  // namespace gloc
