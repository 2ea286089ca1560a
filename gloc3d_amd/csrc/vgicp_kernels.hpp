// vgicp_kernels.hpp -- the device half of the voxelized generalized ICP refinement (gfx950; Koide et al., fast_gicp's
// FastVGICP).  tests/vgicp_ref.py is the contract.
//
//   voxel map of the targets   the voxel map of voxel_map_kernels.hpp (keys, sort, flags, scan, first, hash) with
//                              voxel_stats_kernel here as its statistics kernel: one thread per voxel, fp64 sums relative to the voxel's
//                              corner of its points and of its normals' outer products, in the scan's ORIGINAL order
//   vgicp_accum_kernel         one lane per source point (sorted slot): p = R s + t in fp32 as the other refinements move it,
//                              the voxel p falls into by the fp32 rule of cell_keys_kernel, and per offset of the
//                              neighbourhood one probe of the job's hash table; a voxel found is a pair (N, mu, Nbar): in
//                              fp64 m = R n_s, S = 2I - a (Nbar + m m^T) with a = 1 - plane_eps, M = S^-1 by the symmetric
//                              adjugate, e = p - mu, J = [-[p]x , I], weight N; the 29 sums of a pass, one partial per
//                              work-group through gn6::reduce_store
//
// The 3 x 3 work of a pair is gicp_kernels.hpp's with Nbar in place of n_j n_j^T.  Nbar is a mean of outer products of unit
// (or zero) vectors: symmetric, positive semi-definite, trace <= 1, so S keeps eigenvalues in [2 plane_eps, 2].
//
// Offsets, in the order they are probed and summed (dx, dy, dz):
//   neighbors  1   (0,0,0)
//   neighbors  7   (0,0,0) (-1,0,0) (1,0,0) (0,-1,0) (0,1,0) (0,0,-1) (0,0,1)
//   neighbors 27   dz, dy, dx from -1 to 1 each, dx fastest
//
// KIND (robust.hpp; 0: none, the plain entries' instantiation, whose arithmetic is what it was before there were kinds):
// a pair's s2 = e^T S^-1 e is taken from the adjugate BEFORE the voxel's count rides on M -- (e^T adj e) / det -- and the
// robust weight of the pass's scale then rides on M beside the count; sum w e^T M e stays unweighted by it (N s2) and the
// weights' sum is one more loop-carried accumulator, slot 29.
//
// Registers: with more than one offset the 29 doubles ARE loop-carried (58 registers), unlike the one-pair kernels of
// gn6_kernels.hpp; the loop over the offsets is kept rolled so that one pair's temporaries are live at a time.  The
// compiler's figures are in DESIGN.md.  No floating-point atomics: a lane adds its pairs in offset order, the rest is
// reduce_store's fixed tree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gn6_kernels.hpp"
#include "math3.hpp"  // f32x4, xform, cross3
#include "voxel_map_kernels.hpp"

namespace gloc {
namespace vgicp {

using reg::f32x4;
using gn6::ACC_THREADS;
using gn6::NSLOT;
using gn6::NSUM;
using gn6::State;
using voxmap::KEY_BIAS;
using voxmap::KEY_NONE;

struct Voxel {  // 88 B; the accumulate kernel reads the 80 behind the key
  unsigned long long key;
  uint32_t count, valid;  // valid: count >= min_points (only those are in the hash table)
  double mean[3];
  double nn[6];  // (1 / N) sum n n^T: xx xy xz yy yz zz
};

struct TgtAux {  // beside voxmap::TgtDesc: where a target's normals are
  const uint32_t* inv;  // original index -> position in the normals' order
  const float* nrm;     // packed, zero = none
};

struct Target {  // of a job: its target's hash table and voxels
  const unsigned long long* hkey;
  const uint32_t* hval;
  const Voxel* vox;
  uint32_t mask, pad_;
};

// one thread per voxel (the first of a run of equal keys), as ndt::cell_stats_kernel
static __global__ void voxel_stats_kernel(const voxmap::TgtDesc* __restrict__ tg, const TgtAux* __restrict__ aux,
                                          const unsigned long long* __restrict__ key, const uint32_t* __restrict__ val,
                                          const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, double res,
                                          uint32_t min_pts, Voxel* __restrict__ vox) {
  const voxmap::TgtDesc d = tg[blockIdx.y];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.n || !flag[d.begin + i]) return;
  const TgtAux a = aux[blockIdx.y];
  const unsigned long long k = key[d.begin + i];
  const double cx = (double)((long long)((k >> 42) & 0x1FFFFF) - KEY_BIAS) * res;
  const double cy = (double)((long long)((k >> 21) & 0x1FFFFF) - KEY_BIAS) * res;
  const double cz = (double)((long long)(k & 0x1FFFFF) - KEY_BIAS) * res;
  double s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0};
  uint32_t n = 0;
  for (uint32_t t = i; t < d.n && key[d.begin + t] == k; ++t) {
    const uint32_t j = val[d.begin + t];  // (the sort is stable: ascending original index inside a voxel)
    s1[0] += (double)d.xyz[3 * (size_t)j] - cx;
    s1[1] += (double)d.xyz[3 * (size_t)j + 1] - cy;
    s1[2] += (double)d.xyz[3 * (size_t)j + 2] - cz;
    const size_t o = 3 * (size_t)a.inv[j];
    const double u[3] = {(double)a.nrm[o], (double)a.nrm[o + 1], (double)a.nrm[o + 2]};
    s2[0] += u[0] * u[0]; s2[1] += u[0] * u[1]; s2[2] += u[0] * u[2];
    s2[3] += u[1] * u[1]; s2[4] += u[1] * u[2]; s2[5] += u[2] * u[2];
    ++n;
  }
  Voxel out;
  out.key = k;
  out.count = n;
  out.valid = n >= min_pts ? 1u : 0u;
  const double nd = (double)n;
  out.mean[0] = cx + s1[0] / nd;
  out.mean[1] = cy + s1[1] / nd;
  out.mean[2] = cz + s1[2] / nd;
#pragma unroll
  for (int q = 0; q < 6; ++q) out.nn[q] = s2[q] / nd;
  vox[pos[d.begin + i]] = out;
}

// offset o of the neighbourhood (the order of the header comment)
__device__ __forceinline__ void offset_of(uint32_t neighbors, uint32_t o, int* d) {
  d[0] = 0; d[1] = 0; d[2] = 0;
  if (neighbors == 27u) {
    d[0] = (int)(o % 3u) - 1;
    d[1] = (int)((o / 3u) % 3u) - 1;
    d[2] = (int)(o / 9u) - 1;
  } else if (o > 0u) {
    d[(o - 1u) >> 1] = ((o - 1u) & 1u) ? 1 : -1;
  }
}

template <int KIND>
static __global__ __launch_bounds__(ACC_THREADS) void vgicp_accum_kernel(const gn6::Source* __restrict__ srcs, const Target* __restrict__ tgts,
                                                                         const float* __restrict__ pose_f32, size_t pose_stride /* floats */,
                                                                         const State* __restrict__ states, float inv_res, uint32_t neighbors,
                                                                         double gate2 /* <= 0: off */, double a, bool skip_stopped,
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
    float Tf[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Tf[k] = pose_f32[(size_t)job * pose_stride + k];
    const f32x4 s = S.pts[i];
    float pf[3];
    reg::xform(Tf, s.x, s.y, s.z, pf[0], pf[1], pf[2]);
    // the voxel of p: cell_keys_kernel's rule (a NaN or inf p fails the comparison; so does |k| >= 2^20)
    long long home[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float f = floorf(pf[c] * inv_res);
      ok = ok && fabsf(f) < (float)KEY_BIAS;
      home[c] = ok ? (long long)f : 0;
    }
    if (ok) {
      const double P[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
      const double ns[3] = {(double)S.nrm[3 * (size_t)i], (double)S.nrm[3 * (size_t)i + 1], (double)S.nrm[3 * (size_t)i + 2]};
      double m[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) m[r] = ((double)Tf[3 * r] * ns[0] + (double)Tf[3 * r + 1] * ns[1]) + (double)Tf[3 * r + 2] * ns[2];
      const double mm[6] = {m[0] * m[0], m[0] * m[1], m[0] * m[2], m[1] * m[1], m[1] * m[2], m[2] * m[2]};
      const double c2 = KIND != GLOC_ROBUST_NONE ? gn6::scale2_of(sc, states[job]) : 0.0;
#pragma nounroll
      for (uint32_t o = 0; o < neighbors; ++o) {
        int d[3];
        offset_of(neighbors, o, d);
        const long long kx = home[0] + d[0], ky = home[1] + d[1], kz = home[2] + d[2];
        if (!(kx > -KEY_BIAS && kx < KEY_BIAS && ky > -KEY_BIAS && ky < KEY_BIAS && kz > -KEY_BIAS && kz < KEY_BIAS)) continue;
        const unsigned long long key = voxmap::pack_key(kx, ky, kz);
        uint32_t slot = voxmap::hash_slot(key, T.mask);
        uint32_t ci = 0xFFFFFFFFu;
        while (true) {  // (the table is at most half full: an empty slot ends every probe)
          const unsigned long long hk = T.hkey[slot];
          if (hk == key) {
            ci = T.hval[slot];
            break;
          }
          if (hk == KEY_NONE) break;
          slot = (slot + 1) & T.mask;
        }
        if (ci == 0xFFFFFFFFu) continue;
        const Voxel& V = T.vox[ci];
        const double E[3] = {P[0] - V.mean[0], P[1] - V.mean[1], P[2] - V.mean[2]};
        if (gate2 > 0.0 && !((E[0] * E[0] + E[1] * E[1]) + E[2] * E[2] <= gate2)) continue;
        const double w = (double)V.count;
        // S = 2I - a (Nbar + m m^T), symmetric: xx xy xz yy yz zz
        const double sxx = 2.0 - a * (V.nn[0] + mm[0]), sxy = -a * (V.nn[1] + mm[1]);
        const double sxz = -a * (V.nn[2] + mm[2]), syy = 2.0 - a * (V.nn[3] + mm[3]);
        const double syz = -a * (V.nn[4] + mm[4]), szz = 2.0 - a * (V.nn[5] + mm[5]);
        const double cxx = syy * szz - syz * syz, cxy = sxz * syz - sxy * szz, cxz = sxy * syz - sxz * syy;
        const double cyy = sxx * szz - sxz * sxz, cyz = sxy * sxz - sxx * syz, czz = sxx * syy - sxy * sxy;
        double inv, s2 = 0.0;
        if (KIND == GLOC_ROBUST_NONE) {
          inv = w / ((sxx * cxx + sxy * cxy) + sxz * cxz);  // the weight rides on M
        } else {
          const double inv0 = 1.0 / ((sxx * cxx + sxy * cxy) + sxz * cxz);
          const double ce[3] = {(cxx * E[0] + cxy * E[1]) + cxz * E[2], (cxy * E[0] + cyy * E[1]) + cyz * E[2],
                                (cxz * E[0] + cyz * E[1]) + czz * E[2]};
          s2 = ((E[0] * ce[0] + E[1] * ce[1]) + E[2] * ce[2]) * inv0;
          const double wr = robust::weight<KIND>(s2, c2);
          inv = (w * wr) * inv0;  // the count and the robust weight ride on M
          v[gn6::WSLOT] += wr;
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
        v[0] += W[0][0]; v[1] += W[0][1]; v[2] += W[0][2]; v[3] += A[0][0]; v[4] += A[0][1]; v[5] += A[0][2];
        v[6] += W[1][1]; v[7] += W[1][2]; v[8] += A[1][0]; v[9] += A[1][1]; v[10] += A[1][2];
        v[11] += W[2][2]; v[12] += A[2][0]; v[13] += A[2][1]; v[14] += A[2][2];
        v[15] += M[0][0]; v[16] += M[0][1]; v[17] += M[0][2];
        v[18] += M[1][1]; v[19] += M[1][2];
        v[20] += M[2][2];
        v[21] += gw[0]; v[22] += gw[1]; v[23] += gw[2];
        v[24] += Me[0]; v[25] += Me[1]; v[26] += Me[2];
        if (KIND == GLOC_ROBUST_NONE) {
          v[27] += (E[0] * Me[0] + E[1] * Me[1]) + E[2] * Me[2];
        } else {
          v[27] += w * s2;
        }
        v[28] += 1.0;
      }
    }
  }
  gn6::reduce_store(v, red, partials + ((size_t)S.row0 + blockIdx.x) * NSLOT);
}

}  // namespace vgicp
}  // namespace gloc
